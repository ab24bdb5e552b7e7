"""The fused explicit rollout's adjoint without a GPU: the numpy forward pass of tests/rollout_vjp_ref.py against the
oracle's exact filter, its numpy sweep against central differences of that forward pass (no product code involved), the
product's per-step adjoint (asif_amd/csrc/rollout_vjp_step.hpp compiled for the host behind
tests/host_rollout_vjp_driver.cpp) against that sweep, and the entry's presence in header, binding and library."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import rollout_vjp_ref as ref
from asif_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6
SHAPES = [(1, 1e-3), (8, 1e-2), (40, 1e-3)]


@functools.lru_cache(maxsize=None)
def case(T, dt, keep=0):
    """One batch, its forward pass, the loss weights and the reference sweep; computed once, shared, never written to."""
    oracle_lib.build()
    opt = ref.options(oracle_lib, keep)
    x0, udes = workloads.make_batch(2, B)
    uprev = np.zeros((1, B))
    fw = ref.forward(x0, udes, uprev, T, dt, opt)
    rng = np.random.default_rng(T)
    wxT, wxl, wul = rng.normal(0, 1, (2, B)), rng.normal(0, 1, (T, 2, B)), rng.normal(0, 1, (T, 1, B))
    adj = ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], udes, dt, opt, wxT, None, wxl, wul)
    for a in (x0, udes, uprev, wxT, wxl, wul, *fw.values(), *adj.values()):
        a.setflags(write=False)
    return dict(T=T, dt=dt, opt=opt, x0=x0, udes=udes, uprev=uprev, fw=fw, wxT=wxT, wxl=wxl, wul=wul, adj=adj)


def _loss(c, x0, udes, uprev):
    f = ref.forward(x0, udes, uprev, c["T"], c["dt"], c["opt"])
    # one scalar per instance: instances are independent
    return (c["wxT"] * f["xT"]).sum(axis=0) + (c["wxl"] * f["xlog"]).sum(axis=(0, 1)) + (c["wul"] * f["ulog"]).sum(axis=(0, 1))


@pytest.mark.parametrize("T,dt", SHAPES)
def test_numpy_adjoint_matches_finite_differences_of_the_numpy_rollout(T, dt):
    """Central differences, eps = 1e-6, in both components of x0, in udes and in uact_prev, of a loss with fixed random
    weights on x_T, every xlog[t] and every ulog[t]; bound 1e-6 (1 + |ref|) on all 2048 instances, none left out.
    Measured worst gaps: (1, 1e-3) 7.2e-10, (8, 1e-2) 5.0e-7 (instance 873, d/dx0[0], |ref| up to 141),
    (40, 1e-3) 7.6e-8.  Longer or coarser rollouts cross kinks within eps on a few instances and are not checked."""
    c = case(T, dt)
    e0, e1 = np.array([[1.0], [0.0]]), np.array([[0.0], [1.0]])
    plan = [("x0[0]", c["adj"]["gx0"][0], lambda s: (c["x0"] + s * e0, c["udes"], c["uprev"])),
            ("x0[1]", c["adj"]["gx0"][1], lambda s: (c["x0"] + s * e1, c["udes"], c["uprev"])),
            ("udes", c["adj"]["gudes"][0], lambda s: (c["x0"], c["udes"] + s, c["uprev"])),
            ("uact_prev", c["adj"]["guact0"][0], lambda s: (c["x0"], c["udes"], c["uprev"] + s))]
    for name, g, at in plan:
        fd = (_loss(c, *at(EPS)) - _loss(c, *at(-EPS))) / (2 * EPS)
        gap = np.abs(fd - g) / (1.0 + np.abs(g))
        print(f"T={T} dt={dt} d/d{name}: worst gap {gap.max():.3e} at instance {gap.argmax()} (bound 1e-6)")
        assert gap.max() <= 1e-6, (name, float(gap.max()), int(gap.argmax()))


def test_every_family_of_step_is_there():
    """Failed steps, instances that fail and then recover (or the reverse), steps ending on a safety row, on an input
    bound and free.  (8, 1e-2): 3534 failed steps, 21 mixed instances, 2584 / 3543 / 6723 steps on a row / a bound /
    free; (40, 1e-3): 9 mixed instances."""
    c8, c40, c1 = ref.census(case(8, 1e-2)["fw"]), ref.census(case(40, 1e-3)["fw"]), ref.census(case(1, 1e-3)["fw"])
    msg = f"(1, 1e-3): {c1}; (8, 1e-2): {c8}; (40, 1e-3): {c40}"
    print(msg)
    for cs in (c1, c8, c40):
        assert cs["failed"] > 0 and cs["row"] > 0 and cs["bound"] > 0 and cs["free"] > 0, msg
    assert c8["mixed"] > 0 and c40["mixed"] > 0, msg
    assert c8 == dict(failed=3534, row=2584, bound=3543, free=6723, mixed=21), msg
    assert c40["mixed"] == 9, msg
    assert sum(c8[k] for k in ("failed", "row", "bound", "free")) == 8 * B


@pytest.mark.parametrize("T,dt,keep", [(8, 1e-2, 0), (40, 1e-3, 0), (8, 1e-2, 2)])
def test_reference_forward_is_the_oracles(oracle, T, dt, keep):
    """Step by step, as tests/test_gpu_rollout.py checks the device: the oracle's exact filter on the logged x_t gives the
    logged rc_t and u_t, and the next state is the unfused Euler step of (x_t, u_t) bit for bit."""
    c = case(T, dt, keep)
    fw, u = c["fw"], c["udes"]
    model, variant, o = c["opt"]["oracle"]
    assert np.array_equal(fw["xlog"][0], c["x0"])
    prev_u = c["uprev"][0]
    for t in range(T):
        xt = fw["xlog"][t]
        ua, _, rc = oracle.filter_batch(model, variant, o, np.ascontiguousarray(xt.T), np.ascontiguousarray(u.T),
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


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rolloutvjp") / "librollout_vjp_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_rollout_vjp_driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def run(c, guactT=None, gxlog=True, gulog=True):
        fw, opt = c["fw"], c["opt"]
        o = opt["oracle"][2]
        n = c["x0"].shape[1]
        ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (fw["xlog"], fw["ulog"])]
        rclog = np.ascontiguousarray(fw["rclog"], dtype=np.int32)
        opt_in = [None if a is None else np.ascontiguousarray(a) for a in
                  (guactT, c["wxl"] if gxlog else None, c["wul"] if gulog else None)]
        out = dict(gx0=np.full((2, n), np.nan), gudes=np.full((1, n), np.nan), guact0=np.full((1, n), np.nan),
                   nskip=np.full(n, -77, dtype=np.int32))
        r = lib.rollout_vjp_host_batch(C.c_int64(n), C.c_int32(c["T"]), C.c_double(c["dt"]), C.c_int32(opt["keep"]),
                                       C.c_double(opt["lb"]), C.c_double(opt["ub"]), C.c_double(o.relaxCost),
                                       C.c_double(opt["relaxLb"]), pd(ins[0]), pd(ins[1]),
                                       rclog.ctypes.data_as(C.POINTER(C.c_int32)), pd(np.ascontiguousarray(c["udes"])),
                                       pd(np.ascontiguousarray(c["wxT"])), *[pd(a) for a in opt_in], pd(out["gx0"]),
                                       pd(out["gudes"]), pd(out["guact0"]),
                                       out["nskip"].ctypes.data_as(C.POINTER(C.c_int32)))
        assert r == 0
        return out
    return run


def check_sweep(got, adj, what):
    """The project's VJP bound 1e-9 (1 + |ref|) max(1, 1 / sigma_min) with the sweep's own magnitude S_i in place of |ref|
    (lambda cancels along the sweep) and the smallest active |Lgh| as sigma_min."""
    assert np.all(got["nskip"] == 0), f"{what}: {(got['nskip'] != 0).sum()} instances skipped a solved step"
    scale = (1.0 + adj["S"]) * np.maximum(1.0, 1.0 / adj["amin"])
    worst = 0.0
    for k in ("gx0", "gudes", "guact0"):
        gap = np.abs(got[k] - adj[k]) / scale[None, :]
        print(f"{what} {k}: max scaled gap {gap.max():.3e} (bound 1e-9)")
        assert gap.max() <= 1e-9, (what, k, float(gap.max()), int(gap.max(axis=0).argmax()))
        worst = max(worst, float(gap.max()))
    return worst


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
def test_host_build_of_the_step_matches_the_numpy_sweep(driver, T, dt, keep):
    c = case(T, dt, keep)
    check_sweep(driver(c), c["adj"], f"T={T} dt={dt} keep={keep}")
    if (T, keep) == (8, 0):  # the optional inputs: guactT given, the log gradients absent
        g = np.random.default_rng(5).normal(0, 1, (1, B))
        opt = c["opt"]
        adj = ref.adjoint(c["fw"]["xlog"], c["fw"]["ulog"], c["fw"]["rclog"], c["udes"], dt, opt, c["wxT"], g, None, None)
        check_sweep(driver(c, guactT=g, gxlog=False, gulog=False), adj, "guactT only")


def test_rollout_vjp_entry_is_declared_bound_and_exported():
    name = "asif_hip_rollout_vjp_batch"
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 160
    from asif_amd import capi
    assert name in capi.EXPORTS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load()
    assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 160
    assert hasattr(capi.Filter, "rollout_vjp")
    from asif_amd import torch_layer
    assert hasattr(torch_layer, "ExplicitRolloutFn") and hasattr(torch_layer, "ExplicitRolloutLayer")
