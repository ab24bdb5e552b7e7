"""The cart-driven pendulum (ASIF_HIP_MODEL_CART_PENDULUM) without a GPU: the numpy reference of tests/cart_pendulum_ref.py
against central differences of its own forward pass (no product code involved) -- the first check of the plant term
u_t Dg' lambda, of the row term D2h g + Dh Dg and of the mixed entries of D2h with non-zero values; a census of the step
families; the sensitivity of the reference to those terms; the product's per-step adjoint
(asif_amd/csrc/rollout_params_step.hpp compiled for the host behind tests/host_cart_pendulum_driver.cpp) against the numpy
sweep; and the model's presence in header and binding."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cart_pendulum_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6
SEED = 1010
SHAPES = [(1, 1e-3), (8, 1e-2), (40, 1e-3)]
MAX_LEFT_OUT = (2 * B) // 100  # 2 % of the batch per derivative


def inputs(T, n=B, seed=SEED):
    """x0 in [-1.3, 1.3]^2, k in [-5, 5], K in [-2, 2], v in [-1, 1], alpha in [2, 8], lb in [-5, -3], ub in [3, 5],
    uact_prev in [-1, 1]: drawn for the whole batch, the first n instances returned."""
    rng = np.random.default_rng(seed)
    b = dict(x0=rng.uniform(-1.3, 1.3, (2, B)), k=rng.uniform(-5, 5, (1, B)), K=rng.uniform(-2, 2, (2, B)),
             alpha=rng.uniform(2, 8, B), lb=rng.uniform(-5, -3, (1, B)), ub=rng.uniform(3, 5, (1, B)),
             uprev=rng.uniform(-1, 1, (1, B)))
    b["v"] = np.random.default_rng(seed + T).uniform(-1, 1, (T, 1, B))
    return {k: a[..., :n].copy() for k, a in b.items()}


def weights(T, n=B):
    """Fixed random loss weights: gxT, guactT, gxlog, gulog."""
    rng = np.random.default_rng(2020 + T)
    full = (rng.normal(0, 1, (2, B)), rng.normal(0, 1, (1, B)), rng.normal(0, 1, (T, 2, B)), rng.normal(0, 1, (T, 1, B)))
    return tuple(a[..., :n].copy() for a in full)


@functools.lru_cache(maxsize=None)
def case(T, dt, keep=0, hasK=True, hasV=True, params=("alpha", "lb", "ub")):
    """One batch, its forward pass, the loss weights and the reference sweep; computed once, shared, never written to."""
    opt = ref.options(keep)
    c = inputs(T)
    if not hasK:
        c["K"] = None
    if not hasV:
        c["v"] = None
    for p in ("alpha", "lb", "ub"):
        if p not in params:
            c[p] = None
    fw = ref.forward(c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt, c["alpha"], c["lb"], c["ub"])
    wxT, wuT, wxl, wul = weights(T)
    adj = ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], dt, opt, wxT, wuT, wxl, wul, c["alpha"],
                      c["lb"], c["ub"])
    for a in (*c.values(), wxT, wuT, wxl, wul, *fw.values(), *adj.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(c, T=T, dt=dt, opt=opt, fw=fw, wxT=wxT, wuT=wuT, wxl=wxl, wul=wul, adj=adj)


def _loss(c, fw):
    # one scalar per instance: instances are independent
    return ((c["wxT"] * fw["xT"]).sum(axis=0) + (c["wuT"] * fw["uactT"]).sum(axis=0)
            + (c["wxl"] * fw["xlog"]).sum(axis=(0, 1)) + (c["wul"] * fw["ulog"]).sum(axis=(0, 1)))


@pytest.mark.parametrize("T,dt", SHAPES)
def test_numpy_adjoint_matches_finite_differences_of_the_numpy_rollout(T, dt):
    """Central differences, eps = 1e-6, in both components of x0, k, both entries of K, v[T // 2], alpha, lb, ub and
    uact_prev, of a loss with fixed random weights on x_T, uact_T, every xlog[t] and every ulog[t]; bound
    1e-6 (1 + |ref|).  An instance is left out of a derivative only where one of its two perturbed forward passes differs
    from the unperturbed one in the return code or the working set of some step (a kink within eps); at most 2 % of the
    2048 per derivative.
    Measured, worst gap over the derivatives / most instances left out of one derivative:
    (1, 1e-3) 1.7e-9 (d/dK[1]) / 0;  (8, 1e-2) 6.9e-9 (d/dalpha) / 0;  (40, 1e-3) 2.7e-8 (d/dalpha) / 0."""
    c = case(T, dt)
    sweep, base = c["adj"], c["fw"]

    def fwd(**moved):
        a = {n: moved.get(n, c[n]) for n in ("x0", "k", "K", "v", "uprev", "alpha", "lb", "ub")}
        return ref.forward(a["x0"], a["k"], a["K"], a["v"], a["uprev"], T, dt, c["opt"], a["alpha"], a["lb"], a["ub"])

    def unit(shape, at):
        e = np.zeros(shape)
        e[at] = 1.0
        return e

    t = T // 2
    plan = [("x0[0]", sweep["gx0"][0], "x0", unit((2, 1), (0, 0))), ("x0[1]", sweep["gx0"][1], "x0", unit((2, 1), (1, 0))),
            ("k", sweep["gk"][0], "k", 1.0), ("K[0]", sweep["gK"][0], "K", unit((2, 1), (0, 0))),
            ("K[1]", sweep["gK"][1], "K", unit((2, 1), (1, 0))), (f"v[{t}]", sweep["gv"][t, 0], "v", unit((T, 1, 1), (t, 0, 0))),
            ("alpha", sweep["galpha"], "alpha", 1.0), ("lb", sweep["glb"][0], "lb", 1.0), ("ub", sweep["gub"][0], "ub", 1.0),
            ("uact_prev", sweep["guact0"][0], "uprev", 1.0)]
    for name, g, arg, e in plan:
        up, dn = fwd(**{arg: c[arg] + EPS * e}), fwd(**{arg: c[arg] - EPS * e})
        kink = np.zeros(B, dtype=bool)
        for p in (up, dn):
            kink |= ((p["wid"] != base["wid"]) | (p["rclog"] != base["rclog"])).any(axis=0)
        fd = (_loss(c, up) - _loss(c, dn)) / (2 * EPS)
        gap = np.where(kink, 0.0, np.abs(fd - g) / (1.0 + np.abs(g)))
        print(f"T={T} dt={dt} d/d{name}: worst gap {gap.max():.3e} at instance {gap.argmax()} (bound 1e-6), "
              f"{int(kink.sum())} of {B} left out (cap {MAX_LEFT_OUT})")
        assert kink.sum() <= MAX_LEFT_OUT, (name, int(kink.sum()))
        assert gap.max() <= 1e-6, (name, float(gap.max()), int(gap.argmax()))


CENSUS = {
    (1, 1e-3): dict(failed=477, row=355, bound=268, free=948, mixed=0),
    (8, 1e-2): dict(failed=3766, row=3232, bound=2010, free=7376, mixed=31),
    (40, 1e-3): dict(failed=18930, row=15498, bound=10305, free=37187, mixed=16),
}


def test_every_step_family_is_in_every_shape():
    """Failed, row, bound and free steps at every shape, instances with failed and solved steps at the two longer ones;
    the counts are pinned."""
    got = {s: ref.census(case(*s)["fw"]) for s in SHAPES}
    msg = "; ".join(f"{s}: {c}" for s, c in got.items())
    print(msg)
    for s, cs in got.items():
        assert cs["failed"] > 0 and cs["row"] > 0 and cs["bound"] > 0 and cs["free"] > 0, msg
        assert sum(cs[k] for k in ("failed", "row", "bound", "free")) == s[0] * B
    assert got[(8, 1e-2)]["mixed"] > 0 and got[(40, 1e-3)]["mixed"] > 0, msg
    assert got == CENSUS, msg


def test_the_reference_sees_the_nonlinear_terms():
    """With Dg and the mixed entries of D2h taken as zero the reference's gx0 moves by more than 1e-6 (1 + |ref|) on at
    least 10 % of the instances of shape (8, 1e-2): a sweep that dropped those terms would not pass for this one.
    Measured: 2048 of 2048."""
    c = case(8, 1e-2)
    fw = c["fw"]
    lin = ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], c["dt"], c["opt"], c["wxT"], c["wuT"],
                      c["wxl"], c["wul"], c["alpha"], c["lb"], c["ub"], linearised=True)
    full = c["adj"]["gx0"]
    moved = (np.abs(lin["gx0"] - full) > 1e-6 * (1.0 + np.abs(full))).any(axis=0)
    print(f"gx0 moves on {int(moved.sum())} of {B} instances without Dg and the mixed D2h entries")
    assert moved.sum() >= B // 10, int(moved.sum())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cartpendulum") / "libcart_pendulum_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_cart_pendulum_driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def run(c, gK=True, gv=True, gpar=(True, True, True), guactT=True, gxlog=True, gulog=True):
        fw, opt = c["fw"], c["opt"]
        n, T = c["x0"].shape[1], c["T"]
        cc = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        rclog = np.ascontiguousarray(fw["rclog"], dtype=np.int32)
        ins = [cc(a) for a in (fw["xlog"], fw["ulog"])]
        pol = [cc(c["K"]), cc(c["k"]), cc(c["v"]), cc(c["alpha"]), cc(c["lb"]), cc(c["ub"])]
        gK, gv = gK and c["K"] is not None, gv and c["v"] is not None
        ga, gl, gu = (w and c[n_] is not None for w, n_ in zip(gpar, ("alpha", "lb", "ub")))
        gin = [cc(c["wxT"]), cc(c["wuT"] if guactT else None), cc(c["wxl"] if gxlog else None),
               cc(c["wul"] if gulog else None)]
        nan = lambda *s: np.full(s, np.nan)
        out = dict(gx0=nan(2, n), gK=nan(2, n) if gK else None, gk=nan(1, n), gv=nan(T, 1, n) if gv else None,
                   galpha=nan(n) if ga else None, glb=nan(1, n) if gl else None, gub=nan(1, n) if gu else None,
                   guact0=nan(1, n))
        nskip = np.full(n, -77, dtype=np.int32)
        r = lib.cart_pendulum_vjp_host_batch(C.c_int64(n), C.c_int32(T), C.c_double(c["dt"]), C.c_int32(opt["keep"]),
                                             C.c_double(opt["lb"]), C.c_double(opt["ub"]), C.c_double(opt["relaxCost"]),
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
    """The project's VJP bound 1e-9 (1 + S_i) max(1, 1 / a_min,i): S_i the sweep's own magnitude, a_min,i the smallest
    active |Lgh|; a gradient that was not asked for is not compared.  No instance is left out."""
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


def sweep_of(c, guactT=True, gxlog=True, gulog=True):
    fw = c["fw"]
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], c["dt"], c["opt"], c["wxT"],
                       c["wuT"] if guactT else None, c["wxl"] if gxlog else None, c["wul"] if gulog else None, c["alpha"],
                       c["lb"], c["ub"])


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
def test_host_build_of_the_step_matches_the_numpy_sweep(driver, T, dt, keep):
    """rollout_params_step.hpp on the numpy logs, g++ -ffp-contract=off, every gradient within the bound, nskip 0.
    Measured, worst scaled gap over all shapes and variants: 8.2e-16 of the 1e-9 scale."""
    c = case(T, dt, keep)
    check_sweep(driver(c), c["adj"], f"T={T} dt={dt} keep={keep}")
    if T != 8:
        return
    for hasK, hasV, params in ((False, True, ("alpha", "lb", "ub")), (True, False, ("alpha",)), (False, False, ()),
                               (True, True, ("lb", "ub"))):  # each on its own forward pass
        d = case(T, dt, keep, hasK, hasV, params)
        check_sweep(driver(d), d["adj"], f"K given={hasK}, v given={hasV}, params={params}")
    check_sweep(driver(c, gK=False, gv=False, gpar=(False, False, False)), c["adj"], "no optional gradient requested")
    for only in range(3):
        check_sweep(driver(c, gpar=tuple(j == only for j in range(3))), c["adj"], f"parameter gradient {only} alone")
    check_sweep(driver(c, guactT=False, gxlog=False, gulog=False), sweep_of(c, guactT=False, gxlog=False, gulog=False),
                "gxT only")


def test_model_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    m = re.search(r"\bASIF_HIP_MODEL_CART_PENDULUM\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 10, "ASIF_HIP_MODEL_CART_PENDULUM = 10 not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 190
    from asif_amd import capi
    assert capi.MODEL_CART_PENDULUM == 10 == ref.MODEL
