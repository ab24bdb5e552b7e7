"""The QP solve's vector-Jacobian product without a GPU: the numpy adjoint of tests/qp_vjp_ref.py against central
differences of the oracle's exact solver (no product code involved); the product's adjoint (asif_amd/csrc/qp_vjp_small.hpp
on GiSmall::solve_general<true>, compiled for the host behind tests/host_qp_vjp_driver.cpp, one lane per QP) against that
numpy adjoint; the verdicts of problems the method cannot take; and the entry's presence in header, binding and library.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import qp_vjp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1000
EPS = 1e-6  # the step of tests/test_vjp_ref_host.py
SHAPES = [(2, 4), (2, 18), (3, 17), (3, 41)]
INPUTS = (("Hd", "gHd"), ("c", "gc"), ("A", "gA"), ("b", "gb"), ("lb", "glb"), ("ub", "gub"))
RATIONAL = ("Hd", "A")  # x* is rational in these and piecewise linear in the others


@functools.lru_cache(maxsize=None)
def case(nv, nc, kind):
    """One batch and its reference; computed once, shared, never written to."""
    oracle_lib.build()
    q = ref.family(nv, nc, kind, B)
    r = ref.adjoint(oracle_lib, q)
    for a in (*q.values(), *r.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q, r


def usable(r):
    """Solved and not flagged; a test may leave out flagged instances only, and at most 1 % of a case."""
    ok = r["rc"] == 1
    good = ok & ~r["degenerate"]
    assert (ok & r["degenerate"]).sum() <= 0.01 * len(ok), "more than 1 % of the case is flagged degenerate"
    return good


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("qpvjp") / "libqp_vjp_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_qp_vjp_driver.cpp"), "-o", so])
    lib = C.CDLL(so)

    def run(q):
        nv, nc = q["nv"], q["nc"]
        n = q["c"].shape[0]
        ins = [np.ascontiguousarray(q[k], dtype=np.float64) for k in ("Hd", "c", "A", "b", "lb", "ub")]
        g = np.ascontiguousarray(q["gsol"], dtype=np.float64)
        out = {k: np.full((n, w), np.nan) for k, w in (("gHd", nv), ("gc", nv), ("gA", nv * nc), ("gb", nc), ("glb", nv),
                                                      ("gub", nv), ("sol", nv))}
        rc = np.full(n, -77, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        be = np.ascontiguousarray(q["be"], dtype=np.uint8)
        r = lib.qp_vjp_host_batch(nv, nc, C.c_int64(n), *[p(a) for a in ins], be.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  p(g), *[p(out[k]) for k in (*ref.GRADS, "sol")], rc.ctypes.data_as(C.POINTER(C.c_int32)))
        assert r == 0
        out["rc"] = rc
        return out
    return run


def test_generator_reaches_every_working_set_size():
    """Every instance is solved, the flagged share stays under the cap, and every size of working set from 0 (1 where
    the kind forces a member) to nv occurs among the usable instances of every shape with nc <= 18; on every shape, 3 x 41
    included, some usable instance holds a free variable on its lower and some on its upper bound (3 x 41: 6 and 4 of
    the 3000; 41 rows seldom leave a bound active), so glb and gub are compared on more than zeros.  sigma_min of N D^-1/2 over the usable instances: the smallest of the twelve cases is 0.0048
    (2 x 18 eqrow; the plain and pinned cases stay above 0.008), asserted at 0.004."""
    lowest = 1.0
    for nv, nc in SHAPES:
        bounds = {"glb": 0, "gub": 0}
        for kind in ref.KINDS:
            q, r = case(nv, nc, kind)
            assert np.all(r["rc"] == 1)
            good = usable(r)
            lowest = min(lowest, float(r["smin"][good].min()))
            free = (q["lb"] != q["ub"])[good]  # a pinned variable is in every working set: not what is counted here
            for k in bounds:
                bounds[k] += int(((r[k][good] != 0.0) & free).sum())
            if nc <= 18:
                assert set(r["nactive"][good]) == set(range(0 if kind == "plain" else 1, nv + 1)), (nv, nc, kind)
        print(f"{nv}x{nc}: free variables on a lower / upper bound in {bounds['glb']} / {bounds['gub']} usable instances")
        assert bounds["glb"] > 0 and bounds["gub"] > 0, (nv, nc)
    print(f"smallest sigma_min over the usable instances: {lowest:.4f}")
    assert lowest >= 0.004


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("nv,nc", SHAPES)
def test_numpy_adjoint_matches_finite_differences_of_the_oracle(nv, nc, kind):
    """Per input, one random direction R of +-1 entries over all its components: the central difference of
    L = gsol.x* along R against <gradient, R>, per instance, on all B instances.

    Step and bound are those of tests/test_vjp_ref_host.py: eps = 1e-6 and 1e-8 (1 + |reference|), with no other
    factor.  x* is piecewise linear in c, b, lb and ub, so the central difference has no truncation error there: two
    exact optima, each good to a few ulps of |x*| <= 6, times |gsol| <= 4.5, over 2 eps = 2e-6 -- a dozen ulps come to
    1e-8.  x* is rational in Hd and A, and the central difference then carries a truncation term C eps^2 with C a third
    derivative, of the order of 1 / sigma_min^3: at eps = 1e-6 it reaches 1.2e-8 on 2 x 18 eqrow (instance 475,
    sigma_min 0.009) and 7.5e-9 on 2 x 4 eqrow, and it is a truncation term -- it is 2.9e-9 at eps / 2 and 4.7e-8 at
    2 eps, a factor of four per doubling.  For these two inputs the difference is therefore taken at eps and at 2 eps and
    the eps^2 term removed, (4 d(eps) - d(2 eps)) / 3, which leaves rounding (1.5 times that of one difference) and an
    eps^4 term; the bound stays 1e-8.  Worst over the twelve cases and six inputs after that: 1.5e-9 (3 x 17 pinned, A).

    A variable pinned by lb == ub moves with both its bounds: that derivative is reported on glb (gub = 0), so its lb
    and ub are stepped together when lb is the input, and its ub stays when ub is.
    """
    q, r = case(nv, nc, kind)
    good = usable(r)
    rng = np.random.default_rng(nv * 100 + nc)
    pinned = q["lb"] == q["ub"]

    def central(name, R, eps):
        vals = []
        for s in (+1.0, -1.0):
            qq = dict(q)
            qq[name] = q[name] + s * eps * R
            if name == "lb":
                qq["ub"] = np.where(pinned, qq["lb"], q["ub"])
            x, st = ref.solve(oracle_lib, qq)
            vals.append(((x * q["gsol"]).sum(axis=1), st == 1))
        return (vals[0][0] - vals[1][0]) / (2 * eps), vals[0][1] & vals[1][1]

    for name, gname in INPUTS:
        R = rng.choice([-1.0, 1.0], q[name].shape)
        if name == "ub":
            R[pinned] = 0.0
        fd, same = central(name, R, EPS)
        if name in RATIONAL:
            fd2, same2 = central(name, R, 2 * EPS)
            fd, same = (4.0 * fd - fd2) / 3.0, same & same2
        assert np.all(same[good]), "a stepped instance left the feasible set"
        want = (r[gname] * R).sum(axis=1)
        gap = np.abs(fd - want) / (1.0 + np.abs(want))
        worst = float(gap[good].max())
        print(f"{nv}x{nc} {kind} d/d{name}: max gap {worst:.3e} over {good.sum()} instances, "
              f"{int((want[good] != 0.0).sum())} of them with a gradient")
        assert worst <= 1e-8, (name, worst, int(np.argmax(np.where(good, gap, 0.0))))


def compare(got, r, label):
    """Parity of the product's adjoint with the numpy adjoint: rc on every instance, gradients of the usable ones
    within 1e-9 (1 + |ref|) max(1, 1 / sigma_min), the bound of tests/test_gpu_explicit_vjp.py.  Returns the worst
    scaled gap."""
    assert np.array_equal(got["rc"], r["rc"]), f"{label}: {(got['rc'] != r['rc']).sum()} rc mismatches"
    good = usable(r)
    scale = np.maximum(1.0, 1.0 / r["smin"])[:, None]
    worst = 0.0
    for k in ref.GRADS:
        gap = np.abs(got[k] - r[k]) / ((1.0 + np.abs(r[k])) * scale)
        w = float(gap[good].max())
        worst = max(worst, w)
        assert w <= 1e-9, (label, k, w, int(np.argmax(gap[good].max(axis=1))))
        if k in ("gA", "gb", "glb", "gub"):  # rows and bounds outside the working set: exactly zero
            assert np.all(got[k][good][r[k][good] == 0.0] == 0.0), f"{label} {k}: a gradient outside the working set"
    print(f"{label}: max scaled gap {worst:.3e}")
    return worst


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("nv,nc", SHAPES)
def test_host_build_of_the_adjoint_matches_numpy(driver, nv, nc, kind):
    q, r = case(nv, nc, kind)
    got = driver(q)
    compare(got, r, f"host {nv}x{nc} {kind}")
    assert np.abs(got["sol"] - r["sol"]).max() <= 1e-12


def spoiled(nv, nc):
    """An eqrow batch with every second instance spoiled in one of four ways; returns the batch and the rc expected."""
    q = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in ref.family(nv, nc, "eqrow", 400).items()}
    want = np.ones(400, dtype=np.int32)
    A = q["A"].reshape(400, nv, nc)
    for i in range(1, 400, 2):
        how = (i // 2) % 4
        if how == 0:  # row 1 repeats the equality row 0 with its slack turned to -1: a.x >= b + 1 against a.x == b
            A[i, :, 1] = A[i, :, 0]
            q["b"][i, 1] = q["b"][i, 0] + 1.0
            want[i] = -1
        elif how == 1:
            A[i, i % nv, i % nc] = np.nan
            want[i] = -1
        elif how == 2:
            q["c"][i, i % nv] = np.inf
            want[i] = -1
        else:
            q["Hd"][i, 0] = 0.0
            want[i] = 0
    return q, want


@pytest.mark.parametrize("nv,nc", [(2, 4), (3, 17)])
def test_verdicts_of_problems_the_method_cannot_take(driver, nv, nc):
    """Infeasible (a copy of the equality row with slack -1), a NaN in A, an inf in c: rc -1.  Hd_0 = 0: rc 0.
    All of them: zero gradients.  The instances in between are solved and keep the gradients they have alone."""
    q, want = spoiled(nv, nc)
    got = driver(q)
    assert np.array_equal(got["rc"], want)
    for k in ref.GRADS:
        assert np.all(got[k][want != 1] == 0.0), k
    clean = {k: (v[want == 1] if isinstance(v, np.ndarray) and k != "be" else v) for k, v in q.items()}
    alone = driver(clean)
    for k in (*ref.GRADS, "sol"):
        assert np.array_equal(got[k][want == 1], alone[k]), k


def test_entry_is_declared_bound_and_exported():
    name = "asif_hip_qp_vjp_batch"
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 150
    from asif_amd import capi
    assert name in capi.EXPORTS and hasattr(capi, "qp_vjp_batch")
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT\s+" + name + r"\b", syms), "not exported by the library"
    lib = capi.load()
    assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 150
