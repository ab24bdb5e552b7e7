"""The parameter rollout's adjoint without a GPU: the numpy forward pass of tests/rollout_params_ref.py against the oracle's
exact filter (one call per group of instances that share their parameters) and, with the parameters absent or equal to the
handle's, against tests/rollout_policy_ref.py; its numpy sweep against central differences of that forward pass (no product
code involved); the product's per-step adjoint (asif_amd/csrc/rollout_params_step.hpp compiled for the host behind
tests/host_rollout_params_driver.cpp) against that sweep; and the two entries' presence in header, binding and library."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import rollout_params_ref as ref
import rollout_policy_ref
from asif_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6
SHAPES = [(1, 1e-3), (8, 1e-2), (40, 1e-3)]
MAX_LEFT_OUT = B // 100  # 1 % of the batch per direction and shape
PARAM_SEED = 480         # workloads.uniform: no other batch of the project draws from this seed
TRIPLES = [(2.0, -1.5, 0.5), (4.0, -1.0, 1.0), (6.0, -0.5, 1.5), (8.0, -1.2, 0.8)]  # (alpha, lb, ub) of instance i % 4


def policy_inputs(T, n=B):
    """The gains and the planned sequence of the policy rollout's tests: K ~ (-2, -3) + 0.5 N(0,1), v ~ 0.3 N(0,1)."""
    rng = np.random.default_rng(300)
    K = np.array([[-2.0], [-3.0]]) + 0.5 * rng.normal(0, 1, (2, B))
    v = 0.3 * rng.normal(0, 1, (T, 1, B))
    return K[:, :n].copy(), v[..., :n].copy()


def param_inputs(n=B, first=0):
    """alpha_i in [2, 8], lb_i in [-1.5, -0.5], ub_i in [0.5, 1.5]: alpha [n], lb [1,n], ub [1,n]."""
    i = np.arange(first, first + n, dtype=np.uint64)
    u = lambda j: workloads.uniform(PARAM_SEED, i, j)
    return 2.0 + 6.0 * u(0), (-1.5 + u(1))[None, :].copy(), (0.5 + u(2))[None, :].copy()


def grouped_inputs(n=B):
    t = np.array(TRIPLES)[np.arange(n) % 4]
    return t[:, 0].copy(), t[None, :, 1].copy(), t[None, :, 2].copy()


@functools.lru_cache(maxsize=None)
def case(T, dt, keep=0, hasK=True, hasV=True, params="uniform"):
    """One batch, its forward pass, the loss weights and the reference sweep; computed once, shared, never written to.
    params: "uniform" (param_inputs), "grouped" (TRIPLES), "alpha" (alpha alone), None (all three absent)."""
    oracle_lib.build()
    opt = ref.options(oracle_lib, keep)
    x0, k = workloads.make_batch(2, B)
    K, v = policy_inputs(T)
    K, v = K if hasK else None, v if hasV else None
    alpha, lb, ub = {"uniform": param_inputs, "grouped": grouped_inputs}.get(params, param_inputs)()
    if params == "alpha":
        lb = ub = None
    if params is None:
        alpha = lb = ub = None
    uprev = np.zeros((1, B))
    fw = ref.forward(x0, k, K, v, uprev, T, dt, opt, alpha, lb, ub)
    rng = np.random.default_rng(T)
    wxT, wxl, wul = rng.normal(0, 1, (2, B)), rng.normal(0, 1, (T, 2, B)), rng.normal(0, 1, (T, 1, B))
    adj = ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], k, K, v, dt, opt, wxT, None, wxl, wul, alpha, lb, ub)
    for a in (x0, k, K, v, uprev, alpha, lb, ub, wxT, wxl, wul, *fw.values(), *adj.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(T=T, dt=dt, opt=opt, x0=x0, k=k, K=K, v=v, uprev=uprev, alpha=alpha, lb=lb, ub=ub, fw=fw, wxT=wxT, wxl=wxl,
                wul=wul, adj=adj)


def _loss(c, fw):
    # one scalar per instance: instances are independent
    return ((c["wxT"] * fw["xT"]).sum(axis=0) + (c["wxl"] * fw["xlog"]).sum(axis=(0, 1))
            + (c["wul"] * fw["ulog"]).sum(axis=(0, 1)))


@pytest.mark.parametrize("T,dt", SHAPES)
def test_numpy_adjoint_matches_finite_differences_of_the_numpy_rollout(T, dt):
    """Central differences, eps = 1e-6, in alpha, lb, ub, both components of x0, k, uact_prev, both entries of K and v[t]
    for t = 0, T//2, T-1, of a loss with fixed random weights on x_T, every xlog[t] and every ulog[t]; bound
    1e-6 (1 + |ref|).  An instance is left out of a direction only where its two perturbed forward passes differ from each
    other in the working set or the return code of some step; at most 1 % of the 2048 per direction.
    Measured, worst gap over the directions / most instances left out of one direction:
    (1, 1e-3) 5.5e-10 (d/duact_prev; d/dalpha 4.8e-10) / 0;  (8, 1e-2) 2.9e-9 (d/duact_prev; d/dalpha 2.4e-9) / 0;
    (40, 1e-3) 2.7e-8 (d/dalpha; d/dlb 2.0e-8, d/dub 1.0e-8) / 0."""
    c = case(T, dt)
    sweep = c["adj"]

    def fwd(**moved):
        a = {n: moved.get(n, c[n]) for n in ("x0", "k", "K", "v", "uprev", "alpha", "lb", "ub")}
        return ref.forward(a["x0"], a["k"], a["K"], a["v"], a["uprev"], T, dt, c["opt"], a["alpha"], a["lb"], a["ub"])

    def unit(shape, at):
        e = np.zeros(shape)
        e[at] = 1.0
        return e

    plan = [("alpha", sweep["galpha"], "alpha", 1.0), ("lb", sweep["glb"][0], "lb", 1.0), ("ub", sweep["gub"][0], "ub", 1.0),
            ("x0[0]", sweep["gx0"][0], "x0", unit((2, 1), (0, 0))), ("x0[1]", sweep["gx0"][1], "x0", unit((2, 1), (1, 0))),
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


def test_each_parameter_gradient_has_steps_behind_it():
    """Steps with a nonzero contribution to galpha (on a safety row), to glb and to gub: at least 100 each at (8, 1e-2).
    Measured: (1, 1e-3) row 26, lb 533, ub 517; (8, 1e-2) row 212, lb 4088, ub 4089; (40, 1e-3) row 1098, lb 20662, ub 20457."""
    for s in SHAPES:
        a = case(*s)["adj"]
        print(f"{s}: row {a['nrow']} lb {a['nlb']} ub {a['nub']}")
    a = case(8, 1e-2)["adj"]
    assert a["nrow"] >= 100 and a["nlb"] >= 100 and a["nub"] >= 100, (a["nrow"], a["nlb"], a["nub"])


@pytest.mark.parametrize("T,dt,keep", [(8, 1e-2, 0), (40, 1e-3, 0), (8, 1e-2, 2)])
def test_reference_forward_is_the_oracles(oracle, T, dt, keep):
    """Four groups of instances, each with its own (alpha, lb, ub); step by step and group by group the oracle's exact
    filter with relaxLb, lb, ub set to the group's values gives the logged rc_t and u_t on the logged x_t and the
    reference's uDes_t, and the next state is the unfused Euler step of (x_t, u_t) bit for bit."""
    c = case(T, dt, keep, params="grouped")
    fw = c["fw"]
    model, variant, _ = c["opt"]["oracle"]
    assert np.array_equal(fw["xlog"][0], c["x0"])
    prev_u = c["uprev"][0]
    for t in range(T):
        xt = fw["xlog"][t]
        udes = c["k"][0] + c["K"][0] * xt[0]
        udes = udes + c["K"][1] * xt[1]
        udes = udes + c["v"][t, 0]
        assert np.array_equal(udes, fw["udes"][t])
        for g, (al, lo, hi) in enumerate(TRIPLES):
            o = oracle.default_options(model, variant)
            o.npSSmax = keep
            o.relaxLb, o.lb[0], o.ub[0] = al, lo, hi
            m = np.arange(B) % 4 == g
            ua, _, rc = oracle.filter_batch(model, variant, o, np.ascontiguousarray(xt[:, m].T),
                                            np.ascontiguousarray(udes[m, None]), oracle.SOLVER_EXACT, None, 8,
                                            uact_init=np.ascontiguousarray(prev_u[m, None]))
            assert np.array_equal(fw["rclog"][t][m], rc), f"step {t} group {g}: {(fw['rclog'][t][m] != rc).sum()} rc differ"
            assert np.abs(fw["ulog"][t, 0][m] - ua[:, 0]).max() <= 1e-6
        ut = fw["ulog"][t, 0]
        x0n = xt[0] + dt * ((0.0 + xt[1]) + ut * 0.0)
        x1n = xt[1] + dt * ((0.0 + 0.0) + ut * 1.0)
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        assert np.array_equal(nxt[0], x0n) and np.array_equal(nxt[1], x1n)
        prev_u = ut
    assert np.array_equal(fw["uactT"][0], fw["ulog"][-1, 0])


@pytest.mark.parametrize("T,dt", SHAPES)
def test_default_parameters_are_the_policy_rollout(T, dt):
    """The parameters absent, and present and equal to the handle's defaults: tests/rollout_policy_ref.py's forward pass
    and sweep, bitwise; the parameter gradients are then those of the reference's own formulas and not all zero."""
    c = case(T, dt)
    opt = c["opt"]
    want = rollout_policy_ref.forward(c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt)
    wadj = rollout_policy_ref.adjoint(want["xlog"], want["ulog"], want["rclog"], c["k"], c["K"], c["v"], dt, opt, c["wxT"],
                                      None, c["wxl"], c["wul"])
    full = (np.full(B, opt["relaxLb"]), np.full((1, B), opt["lb"]), np.full((1, B), opt["ub"]))
    for par in ((None, None, None), full):
        got = ref.forward(c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt, *par)
        for name, a in want.items():
            assert np.array_equal(got[name], a), (name, par[0] is None)
        gadj = ref.adjoint(got["xlog"], got["ulog"], got["rclog"], c["k"], c["K"], c["v"], dt, opt, c["wxT"], None,
                           c["wxl"], c["wul"], *par)
        for name in ("gx0", "gk", "gK", "gv", "guact0", "amin"):
            assert np.array_equal(gadj[name], wadj[name]), (name, par[0] is None)
        if par[0] is None:
            assert gadj["galpha"] is None and gadj["glb"] is None and gadj["gub"] is None
        else:
            assert np.any(gadj["galpha"] != 0) and np.any(gadj["glb"] != 0) and np.any(gadj["gub"] != 0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rolloutparams") / "librollout_params_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_rollout_params_driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def run(c, gK=True, gv=True, gpar=(True, True, True), guactT=None, gxlog=True, gulog=True):
        fw, opt = c["fw"], c["opt"]
        o = opt["oracle"][2]
        n, T = c["x0"].shape[1], c["T"]
        cc = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rclog = np.ascontiguousarray(fw["rclog"], dtype=np.int32)
        ins = [cc(a) for a in (fw["xlog"], fw["ulog"])]
        pol = [cc(c["K"]), cc(c["k"]), cc(c["v"]), cc(c["alpha"]), cc(c["lb"]), cc(c["ub"])]
        gK, gv = gK and c["K"] is not None, gv and c["v"] is not None
        ga, gl, gu = (w and c[n_] is not None for w, n_ in zip(gpar, ("alpha", "lb", "ub")))
        gin = [cc(c["wxT"]), cc(guactT), cc(c["wxl"] if gxlog else None), cc(c["wul"] if gulog else None)]
        nan = lambda *s: np.full(s, np.nan)
        out = dict(gx0=nan(2, n), gK=nan(2, n) if gK else None, gk=nan(1, n), gv=nan(T, 1, n) if gv else None,
                   galpha=nan(n) if ga else None, glb=nan(1, n) if gl else None, gub=nan(1, n) if gu else None,
                   guact0=nan(1, n))
        nskip = np.full(n, -77, dtype=np.int32)
        r = lib.rollout_params_vjp_host_batch(C.c_int64(n), C.c_int32(T), C.c_double(c["dt"]), C.c_int32(opt["keep"]),
                                              C.c_double(opt["lb"]), C.c_double(opt["ub"]), C.c_double(o.relaxCost),
                                              C.c_double(opt["relaxLb"]), pd(ins[0]), pd(ins[1]),
                                              rclog.ctypes.data_as(C.POINTER(C.c_int32)), *[pd(a) for a in pol],
                                              *[pd(a) for a in gin], *[pd(a) for a in out.values()],
                                              nskip.ctypes.data_as(C.POINTER(C.c_int32)))
        assert r == 0
        out["nskip"] = nskip
        return out
    return run


GRADS = ("gx0", "gK", "gk", "gv", "galpha", "glb", "gub", "guact0")


def check_sweep(got, adj, what):
    """The project's VJP bound 1e-9 (1 + S_i) max(1, 1 / a_min,i): S_i the sweep's own magnitude (the largest |h_r w_r|
    included), a_min,i the smallest active |Lgh|; a gradient that was not asked for is not compared."""
    assert np.all(got["nskip"] == 0), f"{what}: {(got['nskip'] != 0).sum()} instances skipped a solved step"
    scale = (1.0 + adj["S"]) * np.maximum(1.0, 1.0 / adj["amin"])
    worst = 0.0
    for k in GRADS:
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
                       c["wxl"] if gxlog else None, c["wul"] if gulog else None, c["alpha"], c["lb"], c["ub"])


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
def test_host_build_of_the_step_matches_the_numpy_sweep(driver, T, dt, keep):
    """Measured, worst scaled gap over all shapes and variants: 8.0e-16 of the 1e-9 scale."""
    c = case(T, dt, keep)
    check_sweep(driver(c), c["adj"], f"T={T} dt={dt} keep={keep}")
    if T != 8:
        return
    for hasK, hasV, params in ((False, True, "uniform"), (True, False, "alpha"), (False, False, None),
                               (True, True, "grouped")):  # each on its own forward pass
        d = case(T, dt, keep, hasK, hasV, params)
        check_sweep(driver(d), d["adj"], f"K given={hasK}, v given={hasV}, params={params}")
    check_sweep(driver(c, gK=False, gv=False, gpar=(False, False, False)), c["adj"], "no optional gradient requested")
    for only in range(3):
        check_sweep(driver(c, gpar=tuple(j == only for j in range(3))), c["adj"], f"parameter gradient {only} alone")
    g = np.random.default_rng(5).normal(0, 1, (1, B))
    check_sweep(driver(c, guactT=g, gxlog=False, gulog=False), sweep_of(c, guactT=g, gxlog=False, gulog=False),
                "guactT only")


def test_params_entries_are_declared_bound_and_exported():
    names = ("asif_hip_rollout_params_batch", "asif_hip_rollout_params_vjp_batch")
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 180
    from asif_amd import capi
    for name in names:
        assert name in capi.EXPORTS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load()
    for name in names:
        assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 180
    assert hasattr(capi.Filter, "rollout_params") and hasattr(capi.Filter, "rollout_params_vjp")
    from asif_amd import torch_layer
    assert hasattr(torch_layer, "ParamRolloutFn") and hasattr(torch_layer, "ParamRolloutLayer")
