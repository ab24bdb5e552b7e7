"""The policy rollout's adjoint without a GPU: the numpy forward pass of tests/rollout_policy_ref.py against the oracle's
exact filter and, with the policy switched off, against tests/rollout_vjp_ref.py; its numpy sweep against central
differences of that forward pass (no product code involved); the product's per-step adjoint
(asif_amd/csrc/rollout_policy_step.hpp compiled for the host behind tests/host_rollout_policy_driver.cpp) against that
sweep; and the two entries' presence in header, binding and library."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import rollout_policy_ref as ref
import rollout_vjp_ref
from asif_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6
SHAPES = [(1, 1e-3), (8, 1e-2), (40, 1e-3)]
MAX_LEFT_OUT = B // 100  # 1 % of the batch per direction and shape


def policy_inputs(T, n=B, seed=0):
    """Per-instance gains K ~ (-2, -3) + 0.5 N(0,1) and a planned sequence v ~ 0.3 N(0,1), fixed seeds."""
    rng = np.random.default_rng(300 + seed)
    K = np.array([[-2.0], [-3.0]]) + 0.5 * rng.normal(0, 1, (2, B))
    v = 0.3 * rng.normal(0, 1, (T, 1, B))
    return K[:, :n].copy(), v[..., :n].copy()


@functools.lru_cache(maxsize=None)
def case(T, dt, keep=0, hasK=True, hasV=True):
    """One batch, its forward pass under the policy (without K or v where told so), the loss weights and the reference
    sweep; computed once, shared, never written to."""
    oracle_lib.build()
    opt = ref.options(oracle_lib, keep)
    x0, k = workloads.make_batch(2, B)
    K, v = policy_inputs(T)
    K, v = K if hasK else None, v if hasV else None
    uprev = np.zeros((1, B))
    fw = ref.forward(x0, k, K, v, uprev, T, dt, opt)
    rng = np.random.default_rng(T)
    wxT, wxl, wul = rng.normal(0, 1, (2, B)), rng.normal(0, 1, (T, 2, B)), rng.normal(0, 1, (T, 1, B))
    adj = ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], k, K, v, dt, opt, wxT, None, wxl, wul)
    for a in (x0, k, K, v, uprev, wxT, wxl, wul, *fw.values(), *adj.values()):
        if a is not None:
            a.setflags(write=False)
    return dict(T=T, dt=dt, opt=opt, x0=x0, k=k, K=K, v=v, uprev=uprev, fw=fw, wxT=wxT, wxl=wxl, wul=wul, adj=adj)


def _loss(c, fw):
    # one scalar per instance: instances are independent
    return ((c["wxT"] * fw["xT"]).sum(axis=0) + (c["wxl"] * fw["xlog"]).sum(axis=(0, 1))
            + (c["wul"] * fw["ulog"]).sum(axis=(0, 1)))


@pytest.mark.parametrize("T,dt", SHAPES)
def test_numpy_adjoint_matches_finite_differences_of_the_numpy_rollout(T, dt):
    """Central differences, eps = 1e-6, in both components of x0, in k, in uact_prev, in both entries of K and in v[t] for
    t = 0, T//2, T-1, of a loss with fixed random weights on x_T, every xlog[t] and every ulog[t]; bound 1e-6 (1 + |ref|).
    An instance is left out of a direction only where its two perturbed forward passes differ from each other in the
    working set or the return code of some step (the difference straddles a kink); at most 1 % of the 2048 per direction.
    Measured, worst gap over the directions: (1, 1e-3) 5.5e-10 (d/duact_prev), (8, 1e-2) 2.9e-9 (d/duact_prev),
    (40, 1e-3) 1.4e-8 (d/duact_prev; d/dK 8.0e-9, d/dv 8.8e-9); no instance left out in any direction at any shape."""
    c = case(T, dt)
    sweep = c["adj"]

    def fwd(**moved):
        a = {n: moved.get(n, c[n]) for n in ("x0", "k", "K", "v", "uprev")}
        return ref.forward(a["x0"], a["k"], a["K"], a["v"], a["uprev"], T, dt, c["opt"])

    def unit(shape, at):
        e = np.zeros(shape)
        e[at] = 1.0
        return e

    plan = [("x0[0]", sweep["gx0"][0], "x0", unit((2, 1), (0, 0))), ("x0[1]", sweep["gx0"][1], "x0", unit((2, 1), (1, 0))),
            ("k", sweep["gk"][0], "k", 1.0), ("uact_prev", sweep["guact0"][0], "uprev", 1.0),
            ("K[0]", sweep["gK"][0], "K", unit((2, 1), (0, 0))), ("K[1]", sweep["gK"][1], "K", unit((2, 1), (1, 0)))]
    for t in sorted({0, T // 2, T - 1}):
        plan.append((f"v[{t}]", sweep["gv"][t, 0], "v", unit((T, 1, 1), (t, 0, 0))))
    for name, g, arg, e in plan:
        up, dn = fwd(**{arg: c[arg] + EPS * e}), fwd(**{arg: c[arg] - EPS * e})
        kink = ((up["wid"] != dn["wid"]) | (up["rclog"] != dn["rclog"])).any(axis=0)
        fd = (_loss(c, up) - _loss(c, dn)) / (2 * EPS)
        gap = np.where(kink, 0.0, np.abs(fd - g) / (1.0 + np.abs(g)))
        print(f"T={T} dt={dt} d/d{name}: worst gap {gap.max():.3e} at instance {gap.argmax()} (bound 1e-6), "
              f"{int(kink.sum())} of {B} left out (cap {MAX_LEFT_OUT})")
        assert kink.sum() <= MAX_LEFT_OUT, (name, int(kink.sum()))
        assert gap.max() <= 1e-6, (name, float(gap.max()), int(gap.argmax()))


def test_every_family_of_step_is_there():
    """Failed steps, steps ending on a safety row, on an input bound and free at every shape; instances with both failed
    and solved steps at (8, 1e-2)."""
    cs = {s: ref.census(case(*s)["fw"]) for s in SHAPES}
    msg = "; ".join(f"{s}: {v}" for s, v in cs.items())
    print(msg)
    for v in cs.values():
        assert v["failed"] > 0 and v["row"] > 0 and v["bound"] > 0 and v["free"] > 0, msg
    assert cs[(8, 1e-2)]["mixed"] > 0, msg


@pytest.mark.parametrize("T,dt,keep", [(8, 1e-2, 0), (40, 1e-3, 0), (8, 1e-2, 2)])
def test_reference_forward_is_the_oracles(oracle, T, dt, keep):
    """Step by step: the oracle's exact filter on the logged x_t with the reference's uDes_t gives the logged rc_t and
    u_t, and the next state is the unfused Euler step of (x_t, u_t) bit for bit."""
    c = case(T, dt, keep)
    fw = c["fw"]
    model, variant, o = c["opt"]["oracle"]
    assert np.array_equal(fw["xlog"][0], c["x0"])
    prev_u = c["uprev"][0]
    for t in range(T):
        xt = fw["xlog"][t]
        udes = c["k"][0] + c["K"][0] * xt[0]
        udes = udes + c["K"][1] * xt[1]
        udes = udes + c["v"][t, 0]
        assert np.array_equal(udes, fw["udes"][t])
        ua, _, rc = oracle.filter_batch(model, variant, o, np.ascontiguousarray(xt.T), np.ascontiguousarray(udes[:, None]),
                                        oracle.SOLVER_EXACT, None, 8, uact_init=prev_u[:, None])
        assert np.array_equal(fw["rclog"][t], rc), f"step {t}: rc mismatches {(fw['rclog'][t] != rc).sum()}"
        assert np.abs(fw["ulog"][t, 0] - ua[:, 0]).max() <= 1e-6
        ut = fw["ulog"][t, 0]
        x0n = xt[0] + dt * ((0.0 + xt[1]) + ut * 0.0)
        x1n = xt[1] + dt * ((0.0 + 0.0) + ut * 1.0)
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        assert np.array_equal(nxt[0], x0n) and np.array_equal(nxt[1], x1n)
        prev_u = ut
    assert np.array_equal(fw["uactT"][0], fw["ulog"][-1, 0])


@pytest.mark.parametrize("T,dt", SHAPES)
def test_degenerate_policy_is_the_constant_udes_rollout(T, dt):
    """K = v = None, and K = 0, v = 0: the forward pass of tests/rollout_vjp_ref.py with udes = k, bitwise."""
    c = case(T, dt)
    want = rollout_vjp_ref.forward(c["x0"], c["k"], c["uprev"], T, dt, c["opt"])
    for K, v in ((None, None), (np.zeros((2, B)), np.zeros((T, 1, B)))):
        got = ref.forward(c["x0"], c["k"], K, v, c["uprev"], T, dt, c["opt"])
        for name, a in want.items():
            assert np.array_equal(got[name], a), (name, K is None)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rolloutpolicy") / "librollout_policy_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_rollout_policy_driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def run(c, gK=True, gv=True, guactT=None, gxlog=True, gulog=True):
        fw, opt = c["fw"], c["opt"]
        o = opt["oracle"][2]
        n, T = c["x0"].shape[1], c["T"]
        cc = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rclog = np.ascontiguousarray(fw["rclog"], dtype=np.int32)
        ins = [cc(a) for a in (fw["xlog"], fw["ulog"])]
        pol = [cc(c["K"]), cc(c["k"]), cc(c["v"])]
        gK, gv = gK and c["K"] is not None, gv and c["v"] is not None
        gin = [cc(c["wxT"]), cc(guactT), cc(c["wxl"] if gxlog else None), cc(c["wul"] if gulog else None)]
        out = dict(gx0=np.full((2, n), np.nan), gK=np.full((2, n), np.nan) if gK else None, gk=np.full((1, n), np.nan),
                   gv=np.full((T, 1, n), np.nan) if gv else None, guact0=np.full((1, n), np.nan))
        nskip = np.full(n, -77, dtype=np.int32)
        r = lib.rollout_policy_vjp_host_batch(C.c_int64(n), C.c_int32(T), C.c_double(c["dt"]), C.c_int32(opt["keep"]),
                                              C.c_double(opt["lb"]), C.c_double(opt["ub"]), C.c_double(o.relaxCost),
                                              C.c_double(opt["relaxLb"]), pd(ins[0]), pd(ins[1]),
                                              rclog.ctypes.data_as(C.POINTER(C.c_int32)), *[pd(a) for a in pol],
                                              *[pd(a) for a in gin], *[pd(a) for a in out.values()],
                                              nskip.ctypes.data_as(C.POINTER(C.c_int32)))
        assert r == 0
        out["nskip"] = nskip
        return out
    return run


def check_sweep(got, adj, what):
    """The project's VJP bound 1e-9 (1 + |ref|) max(1, 1 / sigma_min) with the sweep's own magnitude S_i in place of |ref|
    and the smallest active |Lgh| as sigma_min; a gradient that was not asked for is not compared."""
    assert np.all(got["nskip"] == 0), f"{what}: {(got['nskip'] != 0).sum()} instances skipped a solved step"
    scale = (1.0 + adj["S"]) * np.maximum(1.0, 1.0 / adj["amin"])
    worst = 0.0
    for k in ("gx0", "gK", "gk", "gv", "guact0"):
        if got[k] is None:
            continue
        gap = np.abs(got[k] - adj[k]) / scale
        print(f"{what} {k}: max scaled gap {gap.max():.3e} (bound 1e-9)")
        assert gap.max() <= 1e-9, (what, k, float(gap.max()))
        worst = max(worst, float(gap.max()))
    return worst


def sweep_of(c, guactT=None, gxlog=True, gulog=True):
    fw = c["fw"]
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], c["dt"], c["opt"], c["wxT"], guactT,
                       c["wxl"] if gxlog else None, c["wul"] if gulog else None)


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
def test_host_build_of_the_step_matches_the_numpy_sweep(driver, T, dt, keep):
    c = case(T, dt, keep)
    check_sweep(driver(c), c["adj"], f"T={T} dt={dt} keep={keep}")
    if (T, keep) != (8, 0):
        return
    for hasK, hasV in ((False, True), (True, False), (False, False)):  # each on its own forward pass
        d = case(T, dt, keep, hasK, hasV)
        check_sweep(driver(d), d["adj"], f"K given={hasK}, v given={hasV}")
    check_sweep(driver(c, gK=False, gv=False), c["adj"], "gK and gv not requested")
    g = np.random.default_rng(5).normal(0, 1, (1, B))
    check_sweep(driver(c, guactT=g, gxlog=False, gulog=False), sweep_of(c, guactT=g, gxlog=False, gulog=False),
                "guactT only")


def test_policy_entries_are_declared_bound_and_exported():
    names = ("asif_hip_rollout_policy_batch", "asif_hip_rollout_policy_vjp_batch")
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 170
    from asif_amd import capi
    for name in names:
        assert name in capi.EXPORTS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load()
    for name in names:
        assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 170
    assert hasattr(capi.Filter, "rollout_policy") and hasattr(capi.Filter, "rollout_policy_vjp")
    from asif_amd import torch_layer
    assert hasattr(torch_layer, "PolicyRolloutFn") and hasattr(torch_layer, "PolicyRolloutLayer")
