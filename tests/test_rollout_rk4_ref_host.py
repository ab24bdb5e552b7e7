"""The RK4 plant step under a held input and its adjoint without a GPU: the numpy step of tests/rollout_rk4_ref.py against
the exact discretisation of the double integrator and against its own order of convergence on the pendulum; its numpy
sweep against central differences of its own forward pass (no product code involved) on both models; the sensitivity of
that check to the integrator; the product's step and per-step adjoint (asif_amd/csrc/plant_step.hpp and
rollout_params_step.hpp compiled for the host behind tests/host_rollout_rk4_driver.cpp) against the numpy step and sweep;
and the two entries' presence in header, binding and library.

Inputs: the double integrator's are the first 2048 instances of config 2's batch with the policy and parameter draws of
tests/test_rollout_params_ref_host.py, the pendulum's those of tests/test_cart_pendulum_ref_host.py -- imported, not
copied."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cart_pendulum_ref
import oracle_lib
import rollout_params_ref
import rollout_rk4_ref as ref
import test_cart_pendulum_ref_host as cp_inputs
import test_rollout_params_ref_host as di_inputs
from asif_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6
SHAPES = [(1, 1e-3), (8, 1e-2), (40, 1e-3)]
MAX_LEFT_OUT = B // 100  # 1 % of the batch per direction and shape
MODELS = {"di": rollout_params_ref, "cp": cart_pendulum_ref}
MODEL_ID = {"di": 0, "cp": 10}
EPS64 = np.finfo(np.float64).eps


def options(name, keep=0):
    if name == "di":
        oracle_lib.build()
        return rollout_params_ref.options(oracle_lib, keep)
    return cart_pendulum_ref.options(keep)


def inputs(name, T):
    """x0, k, K, v, uprev, alpha, lb, ub and the loss weights wxT, wuT, wxl, wul of one model at one horizon."""
    if name == "di":
        x0, k = workloads.make_batch(2, B)
        K, v = di_inputs.policy_inputs(T)
        alpha, lb, ub = di_inputs.param_inputs()
        rng = np.random.default_rng(T)  # the draws of that file's case(), then one more for uact_T
        wxT, wxl, wul = rng.normal(0, 1, (2, B)), rng.normal(0, 1, (T, 2, B)), rng.normal(0, 1, (T, 1, B))
        return dict(x0=x0, k=k, K=K, v=v, uprev=np.zeros((1, B)), alpha=alpha, lb=lb, ub=ub, wxT=wxT,
                    wuT=rng.normal(0, 1, (1, B)), wxl=wxl, wul=wul)
    c = cp_inputs.inputs(T)
    wxT, wuT, wxl, wul = cp_inputs.weights(T)
    return dict(c, wxT=wxT, wuT=wuT, wxl=wxl, wul=wul)


@functools.lru_cache(maxsize=None)
def case(name, T, dt, keep=0, hasK=True, hasV=True, params=True):
    """One batch, its RK4 forward pass, the loss weights and the reference sweep; computed once, shared, never written."""
    mod, opt = MODELS[name], options(name, keep)
    c = inputs(name, T)
    if not hasK:
        c["K"] = None
    if not hasV:
        c["v"] = None
    if not params:
        c["alpha"] = c["lb"] = c["ub"] = None
    fw = ref.forward(mod, c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt, c["alpha"], c["lb"], c["ub"])
    adj = ref.adjoint(mod, fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], dt, opt, c["wxT"], c["wuT"], c["wxl"],
                      c["wul"], c["alpha"], c["lb"], c["ub"])
    for a in (*c.values(), *fw.values(), *adj.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(c, name=name, mod=mod, T=T, dt=dt, opt=opt, fw=fw, adj=adj)


def _loss(c, fw):
    # one scalar per instance: instances are independent
    return ((c["wxT"] * fw["xT"]).sum(axis=0) + (c["wuT"] * fw["uactT"]).sum(axis=0)
            + (c["wxl"] * fw["xlog"]).sum(axis=(0, 1)) + (c["wul"] * fw["ulog"]).sum(axis=(0, 1)))


def test_rk4_is_the_exact_held_input_step_of_the_double_integrator():
    """x1 + dt x2 + dt^2 u / 2, x2 + dt u within 8 eps (1 + |x|); the Euler step misses x1 by dt^2 |u| / 2 to the same
    bound and agrees in x2.  Measured: RK4 1.1e-16 (1 + |x|) at worst, the Euler gap off dt^2 |u| / 2 by 1.1e-16."""
    x, _ = workloads.make_batch(2, B)
    u = np.random.default_rng(7).uniform(-1, 1, B)
    for dt in (1e-3, 1e-2, 0.1):
        exact = np.stack([x[0] + dt * x[1] + dt * dt * u / 2.0, x[1] + dt * u])
        bound = 8 * EPS64 * (1.0 + np.abs(exact))
        got = ref.rk4_step(rollout_params_ref, x, u, dt)
        print(f"dt={dt}: RK4 worst {(np.abs(got - exact) / (1.0 + np.abs(exact))).max():.2e}")
        assert np.all(np.abs(got - exact) <= bound)
        eul = ref.euler_step(rollout_params_ref, x, u, dt)
        gap = np.abs(eul - exact)
        assert np.all(np.abs(gap[0] - dt * dt * np.abs(u) / 2.0) <= bound[0])
        assert np.all(gap[1] <= bound[1])
        assert np.any(gap[0] > bound[0])


def _plant_error(step, dt, horizon, x0, u):
    x = x0.copy()
    for _ in range(int(round(horizon / dt))):
        x = step(cart_pendulum_ref, x, u, dt)
    fine = x0.copy()
    for _ in range(int(round(horizon / dt)) * 64):
        fine = ref.rk4_step(cart_pendulum_ref, fine, u, dt / 64)
    return np.sqrt(((x - fine) ** 2).sum())


def test_order_of_convergence_on_the_pendulum():
    """The plant alone under a constant input over a horizon of 1.6, against the same RK4 at dt / 64: halving dt divides
    the error (2-norm over 256 instances) by 12 to 20 for RK4 and by 1.7 to 2.3 for the Euler step, at dt = 0.1 and 0.05
    -- the theoretical 16 and 2 with room for the next-order term.
    Measured: RK4 15.7 and 15.8, Euler 1.97 and 1.99."""
    rng = np.random.default_rng(11)
    x0, u = rng.uniform(-1.0, 1.0, (2, 256)), rng.uniform(-1.0, 1.0, 256)
    for step, lo, hi in ((ref.rk4_step, 12.0, 20.0), (ref.euler_step, 1.7, 2.3)):
        e = [_plant_error(step, dt, 1.6, x0, u) for dt in (0.1, 0.05, 0.025)]
        ratios = (e[0] / e[1], e[1] / e[2])
        print(f"{step.__name__}: errors {e}, ratios {ratios}")
        assert all(lo <= r <= hi for r in ratios), (step.__name__, ratios)


@pytest.mark.parametrize("T,dt", SHAPES)
@pytest.mark.parametrize("name", ["di", "cp"])
def test_numpy_adjoint_matches_finite_differences_of_the_numpy_rollout(name, T, dt):
    """Central differences, eps = 1e-6, in both components of x0, k, both entries of K, v[t] for t = 0, T//2, T-1, alpha,
    lb, ub and uact_prev, of a loss with fixed random weights on x_T, uact_T, every xlog[t] and every ulog[t]; bound
    1e-6 (1 + |ref|).  An instance is left out of a direction only where its two perturbed forward passes differ from each
    other in the working set or the return code of some step; at most 1 % of the 2048 per direction and shape.
    Measured, worst gap over the directions / most instances left out of one direction:
    di (1, 1e-3) 5.2e-10 (d/duact_prev) / 0;  (8, 1e-2) 3.0e-9 (d/dK[0]) / 0;  (40, 1e-3) 1.1e-8 (d/dx0[1]) / 0;
    cp (1, 1e-3) 1.5e-9 (d/dK[1]) / 0;  (8, 1e-2) 1.0e-8 (d/dalpha) / 0;  (40, 1e-3) 2.9e-8 (d/dalpha) / 0."""
    c = case(name, T, dt)
    sweep = c["adj"]

    def fwd(**moved):
        a = {n: moved.get(n, c[n]) for n in ("x0", "k", "K", "v", "uprev", "alpha", "lb", "ub")}
        return ref.forward(c["mod"], a["x0"], a["k"], a["K"], a["v"], a["uprev"], T, dt, c["opt"], a["alpha"], a["lb"],
                           a["ub"])

    def unit(shape, at):
        e = np.zeros(shape)
        e[at] = 1.0
        return e

    plan = [("x0[0]", sweep["gx0"][0], "x0", unit((2, 1), (0, 0))), ("x0[1]", sweep["gx0"][1], "x0", unit((2, 1), (1, 0))),
            ("k", sweep["gk"][0], "k", 1.0), ("K[0]", sweep["gK"][0], "K", unit((2, 1), (0, 0))),
            ("K[1]", sweep["gK"][1], "K", unit((2, 1), (1, 0))), ("alpha", sweep["galpha"], "alpha", 1.0),
            ("lb", sweep["glb"][0], "lb", 1.0), ("ub", sweep["gub"][0], "ub", 1.0),
            ("uact_prev", sweep["guact0"][0], "uprev", 1.0)]
    for t in sorted({0, T // 2, T - 1}):
        plan.append((f"v[{t}]", sweep["gv"][t, 0], "v", unit((T, 1, 1), (t, 0, 0))))
    for what, g, arg, e in plan:
        up, dn = fwd(**{arg: c[arg] + EPS * e}), fwd(**{arg: c[arg] - EPS * e})
        kink = ((up["wid"] != dn["wid"]) | (up["rclog"] != dn["rclog"])).any(axis=0)
        fd = (_loss(c, up) - _loss(c, dn)) / (2 * EPS)
        with np.errstate(invalid="ignore"):
            gap = np.where(kink, 0.0, np.abs(fd - g) / (1.0 + np.abs(g)))
        print(f"{name} T={T} dt={dt} d/d{what}: worst gap {gap.max():.3e} at instance {gap.argmax()} (bound 1e-6), "
              f"{int(kink.sum())} of {B} left out (cap {MAX_LEFT_OUT})")
        assert kink.sum() <= MAX_LEFT_OUT, (what, int(kink.sum()))
        assert gap.max() <= 1e-6, (what, float(gap.max()), int(gap.argmax()))


CENSUS = {
    ("di", 1, 1e-3): dict(failed=483, row=26, bound=1050, free=489),
    ("di", 8, 1e-2): dict(failed=3786, row=212, bound=8177, free=4209),
    ("di", 40, 1e-3): dict(failed=19153, row=1098, bound=41119, free=20550),
    ("cp", 1, 1e-3): dict(failed=477, row=355, bound=268, free=948),
    ("cp", 8, 1e-2): dict(failed=3767, row=3233, bound=2009, free=7375),
    ("cp", 40, 1e-3): dict(failed=18929, row=15499, bound=10305, free=37187),
}


def test_every_step_family_is_behind_the_check():
    """The census of failed / row / bound / free steps of the RK4 forward passes, pinned; at (8, 1e-2) at least 100 steps
    of each solved kind on either model."""
    got = {(n, *s): ref.census(case(n, *s)["fw"]) for n in MODELS for s in SHAPES}
    msg = "; ".join(f"{s}: {c}" for s, c in got.items())
    print(msg)
    for n in MODELS:
        cs = got[(n, 8, 1e-2)]
        assert cs["row"] >= 100 and cs["bound"] >= 100 and cs["free"] >= 100, msg
    assert got == CENSUS, msg


SWITCH_SHARE = 2048  # measured: every instance


def test_the_check_tells_the_integrators_apart():
    """The Euler adjoint of the plant on the RK4 logs (the reference's switch) moves gx0 by more than 1e-6 (1 + |ref|) on
    the pinned number of the pendulum's 2048 instances at (8, 1e-2): a sweep that ignored the integrator would not pass
    for this one."""
    c = case("cp", 8, 1e-2)
    fw = c["fw"]
    eul = ref.adjoint(c["mod"], fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], c["dt"], c["opt"], c["wxT"],
                      c["wuT"], c["wxl"], c["wul"], c["alpha"], c["lb"], c["ub"], plant="euler")
    full = c["adj"]["gx0"]
    moved = (np.abs(eul["gx0"] - full) > 1e-6 * (1.0 + np.abs(full))).any(axis=0)
    print(f"gx0 moves beyond the bound on {int(moved.sum())} of {B}")
    assert int(moved.sum()) == SWITCH_SHARE
    assert moved.sum() >= B // 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rolloutrk4") / "librollout_rk4_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_rollout_rk4_driver.cpp"), "-o", so])
    lib = C.CDLL(so)
    pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def step(name, x, u, dt):
        x, u = np.ascontiguousarray(x), np.ascontiguousarray(u)
        xn = np.full_like(x, np.nan)
        assert lib.plant_step_host_batch(C.c_int32(MODEL_ID[name]), C.c_int64(x.shape[1]), C.c_double(dt), pd(x), pd(u),
                                         pd(xn)) == 0
        return xn

    def sweep(c, integrator=1, gK=True, gv=True, gpar=(True, True, True), guactT=True, gxlog=True, gulog=True):
        fw, opt = c["fw"], c["opt"]
        relax_cost = opt["oracle"][2].relaxCost if c["name"] == "di" else opt["relaxCost"]
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
        r = lib.rollout_rk4_vjp_host_batch(C.c_int32(MODEL_ID[c["name"]]), C.c_int32(integrator), C.c_int64(n), C.c_int32(T),
                                           C.c_double(c["dt"]), C.c_int32(opt["keep"]), C.c_double(opt["lb"]),
                                           C.c_double(opt["ub"]), C.c_double(relax_cost), C.c_double(opt["relaxLb"]),
                                           pd(ins[0]), pd(ins[1]), rclog.ctypes.data_as(C.POINTER(C.c_int32)),
                                           *[pd(a) for a in pol], *[pd(a) for a in gin], *[pd(a) for a in out.values()],
                                           nskip.ctypes.data_as(C.POINTER(C.c_int32)))
        assert r == 0
        out["nskip"] = nskip
        return out
    return step, sweep


@pytest.mark.parametrize("name", ["di", "cp"])
def test_host_build_of_the_plant_step_is_the_numpy_step(driver, name):
    """plant_step.hpp (the RK4 step) from (x, u): bitwise on the double integrator; on the pendulum within
    1e-14 (1 + |x|) (the host's sine and cosine are numpy's here: measured 0)."""
    step, _ = driver
    c = case(name, 8, 1e-2)
    x, u = c["fw"]["xlog"][3], c["fw"]["ulog"][3]
    for dt in (1e-3, 1e-2):
        got, exp = step(name, x, u, dt), ref.rk4_step(c["mod"], x, u[0], dt)
        if name == "di":
            assert np.array_equal(got, exp), dt
        else:
            gap = np.abs(got - exp) / (1.0 + np.abs(exp))
            print(f"cp dt={dt}: worst {gap.max():.2e}")
            assert gap.max() <= 1e-14


GRADS = ("gx0", "gK", "gk", "gv", "galpha", "glb", "gub", "guact0")


def check_sweep(got, adj, what):
    """The project's VJP bound 1e-9 (1 + S_i) max(1, 1 / a_min,i): S_i the sweep's own magnitude, the stage adjoints
    included, a_min,i the smallest active |Lgh|; a gradient that was not asked for is not compared."""
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


def sweep_of(c, guactT=True, gxlog=True, gulog=True, plant="rk4"):
    fw = c["fw"]
    return ref.adjoint(c["mod"], fw["xlog"], fw["ulog"], fw["rclog"], c["k"], c["K"], c["v"], c["dt"], c["opt"], c["wxT"],
                       c["wuT"] if guactT else None, c["wxl"] if gxlog else None, c["wul"] if gulog else None, c["alpha"],
                       c["lb"], c["ub"], plant=plant)


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
@pytest.mark.parametrize("name", ["di", "cp"])
def test_host_build_of_the_step_matches_the_numpy_sweep(driver, name, T, dt, keep):
    """npSSmax 0 and 2, nskip 0 everywhere; at T = 8 also with K, v, the parameters, the optional gradients and the
    optional loss terms absent, and the Euler instantiation against the reference's Euler sweep on the same logs.
    Measured, worst scaled gap over all shapes and variants: 1.1e-15 of the 1e-9 scale."""
    _, sweep = driver
    c = case(name, T, dt, keep)
    check_sweep(sweep(c), c["adj"], f"{name} T={T} dt={dt} keep={keep}")
    if T != 8:
        return
    for hasK, hasV, params in ((False, True, True), (True, False, True), (False, False, False), (True, True, False)):
        d = case(name, T, dt, keep, hasK, hasV, params)  # each on its own forward pass
        check_sweep(sweep(d), d["adj"], f"{name} K given={hasK}, v given={hasV}, params={params}")
    check_sweep(sweep(c, gK=False, gv=False, gpar=(False, False, False)), c["adj"], "no optional gradient requested")
    for only in range(3):
        check_sweep(sweep(c, gpar=tuple(j == only for j in range(3))), c["adj"], f"parameter gradient {only} alone")
    check_sweep(sweep(c, guactT=False, gxlog=False, gulog=False), sweep_of(c, False, False, False), "gxT only")
    check_sweep(sweep(c, integrator=0), sweep_of(c, plant="euler"), "the Euler instantiation on the same logs")


def test_sanitizer_program_builds_and_runs(tmp_path):
    """tests/host_rollout_rk4_driver.cpp with -DRK4_DRIVER_MAIN is a program of its own: both models, both integrators,
    every combination of absent inputs and outputs, under AddressSanitizer and UBSan on the CPU."""
    exe = str(tmp_path / "rk4_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRK4_DRIVER_MAIN", "-I" + os.path.join(ROOT, "asif_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_rollout_rk4_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert re.match(r"checksum -?\d", out.stdout) and "nan" not in out.stdout, out.stdout


def test_plant_entries_are_declared_bound_and_exported():
    names = ("asif_hip_rollout_plant_batch", "asif_hip_rollout_plant_vjp_batch")
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 200
    assert re.search(r"#define ASIF_HIP_PLANT_EULER\s+0\b", header) and re.search(r"#define ASIF_HIP_PLANT_RK4\s+1\b", header)
    from asif_amd import capi
    for name in names:
        assert name in capi.EXPORTS
    assert (capi.PLANT_EULER, capi.PLANT_RK4) == (0, 1)
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load()
    for name in names:
        assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 200
    assert hasattr(capi.Filter, "rollout_plant") and hasattr(capi.Filter, "rollout_plant_vjp")
    import inspect
    from asif_amd import torch_layer
    for cls in (torch_layer.PolicyRolloutFn, torch_layer.ParamRolloutFn):
        assert inspect.signature(cls.forward).parameters["integrator"].default == "euler"
    for cls in (torch_layer.PolicyRolloutLayer, torch_layer.ParamRolloutLayer):
        assert inspect.signature(cls.__init__).parameters["integrator"].default == "euler"
