"""asif_hip_rollout_plant_batch / asif_hip_rollout_plant_vjp_batch (asif_amd/csrc/k_rollout_plant.hip) and the torch layers'
integrator argument: the fused rollout under an affine policy with the plant stepped by forward Euler or by RK4 under a
held input, on the double integrator and on the cart-driven pendulum.

ASIF_HIP_PLANT_EULER: the params entries bit for bit, forward and backward.  ASIF_HIP_PLANT_RK4: every forward step
checked on the device's own logs against the references' filter step and the numpy step of tests/rollout_rk4_ref.py; the
backward pass against that file's sweep (itself checked against finite differences in tests/test_rollout_rk4_ref_host.py)
on the device's logs, within 1e-9 (1 + S_i) max(1, 1 / a_min,i) with S_i extended over the stage adjoints.  Buffers,
batches and loss weights are those of tests/test_gpu_rollout_params.py and tests/test_gpu_cart_pendulum.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cart_pendulum_ref
import oracle_lib
import rollout_params_ref
import rollout_rk4_ref as ref
import test_gpu_cart_pendulum as cpt
import test_gpu_rollout_params as par
import test_gpu_rollout_policy as pol
from asif_amd import workloads

pytestmark = pytest.mark.gpu

DEV, NB, SENTINEL, GRADS = pol.DEV, pol.NB, pol.SENTINEL, par.GRADS
view = pol.view
EUNSUPPORTED, EINVAL = -3, -1
EULER, RK4 = 0, 1
EPS64 = np.finfo(np.float64).eps
MODELS = ("di", "cp")
MOD = {"di": rollout_params_ref, "cp": cart_pendulum_ref}
SHAPES = [(1, 1e-3, 1, 1), (8, 1e-2, 65, 192), (1, 1e-3, NB, NB), (8, 1e-2, NB, NB), (40, 1e-3, NB, NB)]


class Plant:
    """A filter whose rollout_params / rollout_params_vjp are the plant entries under one integrator: the launch helpers
    of the params tests then drive the new entries unchanged."""

    def __init__(self, flt, integrator):
        self.flt, self.integrator = flt, integrator

    def rollout_params(self, T, dt, *a, **kw):
        return self.flt.rollout_plant(T, dt, self.integrator, *a, **kw)

    def rollout_params_vjp(self, T, dt, *a, **kw):
        return self.flt.rollout_plant_vjp(T, dt, self.integrator, *a, **kw)


def make_filter(hip, name, keep=0, **solver):
    model = hip.MODEL_DOUBLE_INTEGRATOR if name == "di" else hip.MODEL_CART_PENDULUM
    od = hip.default_options(model, hip.EXPLICIT)
    od.npSSmax = keep
    return hip.Filter(model, hip.EXPLICIT, options=od, solver=hip.default_solver(**solver) if solver else None)


def batch(name, T, n=NB, **kw):
    return par.batch(T, n, **kw) if name == "di" else cpt.batch(T, n, **kw)


def weights(name, T, n=NB):
    if name == "cp":
        return cpt.weights(T, n)
    return pol.weights(T, n)


def options(name, keep=0):
    if name == "di":
        oracle_lib.build()
        return rollout_params_ref.options(oracle_lib, keep)
    return cart_pendulum_ref.options(keep)


def reference(name, fw, b, dt, keep, gxT, guactT=None, gxlog=None, gulog=None):
    return ref.adjoint(MOD[name], fw["xlog"], fw["ulog"], fw["rclog"], b["k"], b["K"], b["v"], dt, options(name, keep), gxT,
                       guactT, gxlog, gulog, b["alpha"], b["lb"], b["ub"])


@pytest.mark.parametrize("T,dt,n,ld", SHAPES)
@pytest.mark.parametrize("name", MODELS)
def test_euler_is_the_params_entries_bit_for_bit(hip, name, T, dt, n, ld):
    """integrator = EULER, forward and backward, every output and the padding."""
    flt = make_filter(hip, name)
    b, g = batch(name, T, n), weights(name, T, n)
    want = par.forward(flt, b, T, dt, ld)
    got = par.forward(Plant(flt, EULER), b, T, dt, ld)
    for k, a in want.items():
        assert np.array_equal(got[k], a), k
    wantg = par.backward(flt, want, b, T, dt, *g, ld=ld)
    gotg = par.backward(Plant(flt, EULER), want, b, T, dt, *g, ld=ld)
    for k, a in wantg.items():
        assert np.array_equal(gotg[k], a), k
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2)])
@pytest.mark.parametrize("name", MODELS)
def test_rk4_forward_step_by_step_on_the_device_logs(hip, name, T, dt, n, ld, keep):
    """On xlog[t]: rclog[t] is the reference filter's verdict (on the pendulum a difference is allowed only within 1e-12
    of the reference's threshold, at most one step in a thousand), ulog[t] within 1e-9 (1 + |u|), and the step from
    (xlog[t], ulog[t]) to xlog[t+1] is the numpy RK4 step: bit for bit on the double integrator, within 1e-14 (1 + |x|)
    on the pendulum.  On the double integrator the logged steps also satisfy the exact held-input discretisation within
    8 eps (1 + |x|)."""
    mod = MOD[name]
    flt = make_filter(hip, name, keep)
    b = batch(name, T, n)
    fw = par.forward(Plant(flt, RK4), b, T, dt, ld)
    opt = options(name, keep)
    lane = mod.lane_params(opt, n, b["alpha"], b["lb"], b["ub"])
    assert np.array_equal(fw["xlog"][0], b["x0"])
    budget, worst_u, worst_x = [0], 0.0, 0.0
    prev = b["uprev"][0]
    for t in range(T):
        xt, ut, rc = fw["xlog"][t], fw["ulog"][t, 0], fw["rclog"][t]
        s = mod.filter_step(xt, mod.policy(b["k"], b["K"], b["v"][t], xt), opt["keep"], *lane)
        if name == "cp":
            same = cpt.rc_agrees(rc, s, f"step {t}", budget)
        else:
            assert np.array_equal(rc, np.where(s["ok"], 1, -1)), f"step {t}"
            same = np.ones(n, dtype=bool)
        want = np.where(rc == 1, s["u"], prev)
        worst_u = max(worst_u, float((np.abs(ut - want) / (1.0 + np.abs(want)))[same].max()))
        assert np.array_equal(ut[rc < 0], prev[rc < 0]), f"step {t}: a failed step moved u"
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        with np.errstate(invalid="ignore", over="ignore"):
            step = ref.rk4_step(mod, xt, ut, dt)
        if name == "di":
            assert np.array_equal(nxt, step), f"step {t}: {(nxt != step).sum()} entries differ from the numpy RK4 step"
            exact = np.stack([xt[0] + dt * xt[1] + dt * dt * ut / 2.0, xt[1] + dt * ut])
            assert np.all(np.abs(nxt - exact) <= 8 * EPS64 * (1.0 + np.abs(exact))), f"step {t}"
        else:
            worst_x = max(worst_x, float((np.abs(nxt - step) / (1.0 + np.abs(step))).max()))
        prev = ut
    print(f"{name} T={T} dt={dt} B={n} keep={keep}: {budget[0]} return codes excepted; max u gap {worst_u:.3e} (bound 1e-9); "
          f"max RK4 step gap {worst_x:.3e} (bound 1e-14)")
    assert budget[0] <= max(1, (T * n) // 1000) and worst_u <= 1e-9 and worst_x <= 1e-14
    assert np.array_equal(fw["nfail"], (fw["rclog"] < 0).sum(axis=0))
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2)])
@pytest.mark.parametrize("name", MODELS)
def test_rk4_sweep_matches_reference_on_device_logs(hip, name, T, dt, n, ld, keep):
    """Every gradient within the bound, nskip 0, padding and sentinels untouched, every slot i < B written."""
    flt = make_filter(hip, name, keep)
    b, g = batch(name, T, n), weights(name, T, n)
    fw = par.forward(Plant(flt, RK4), b, T, dt, ld)
    got = par.backward(Plant(flt, RK4), fw, b, T, dt, *g, ld=ld)
    par.check_parity(got, reference(name, fw, b, dt, keep, *g), n, f"{name} T={T} dt={dt} B={n} ld={ld} keep={keep}")
    for k in GRADS:
        assert np.all(got[k][..., n:] == SENTINEL), f"{k}: slots >= B written"
        assert not np.any(got[k][..., :n] == SENTINEL), f"{k}: a slot < B not written"
    assert np.all(got["nskip"][n:] == -77)
    flt.close()


@pytest.mark.parametrize("name", MODELS)
def test_rk4_every_optional_input_and_gradient(hip, name):
    """K, v, each parameter, guactT, gxlog, gulog and the optional gradients present and absent -- the combination classes
    of the params tests; a smaller batch against the prefix of a larger one, bit for bit."""
    T, dt = 8, 1e-2
    flt = make_filter(hip, name)
    p = Plant(flt, RK4)
    g = weights(name, T)
    for hasK, hasV, params in ((False, True, par.PARAMS), (True, False, ("alpha",)), (True, True, ("lb",)),
                               (True, True, ("ub",)), (False, False, ())):
        b = batch(name, T, hasK=hasK, hasV=hasV, params=params)
        fw = par.forward(p, b, T, dt)
        par.check_parity(par.backward(p, fw, b, T, dt, *g), reference(name, fw, b, dt, 0, *g), NB,
                         f"{name} K={hasK} v={hasV} params={params}")
    b = batch(name, T)
    fw = par.forward(p, b, T, dt)
    for gg, what in (((g[0], None, None, None), "gxT alone"), ((g[0], g[1], None, None), "no log gradients"),
                     ((g[0], None, g[2], None), "gxlog"), ((g[0], None, None, g[3]), "gulog")):
        par.check_parity(par.backward(p, fw, b, T, dt, *gg), reference(name, fw, b, dt, 0, *gg), NB, f"{name} {what}")
    full = par.backward(p, fw, b, T, dt, *g)
    got = par.backward(p, fw, b, T, dt, *g, gK=False, gv=False, gpar=False)
    for k in ("gx0", "gk", "guact0", "nskip"):
        assert np.array_equal(got[k], full[k]), k
    m = 100
    bs, gs = batch(name, T, m), tuple(a[..., :m] for a in g)
    fs = par.forward(p, bs, T, dt)
    for k, a in fs.items():
        assert np.array_equal(a, fw[k][..., :m]), k
    small = par.backward(p, fs, bs, T, dt, *gs)
    for k in GRADS + ("nskip",):
        assert np.array_equal(small[k], full[k][..., :m]), k
    flt.close()


@pytest.mark.parametrize("name", MODELS)
def test_rk4_identities_chaining_and_bad_parameters(hip, name):
    """T = 0 is the identity and B = 0 returns OK; two chained segments (3 + 5 steps) against one of 8: forward, gx0 and
    guact0 (and gv) bit for bit, the sums gk, gK, galpha, glb, gub -- taken in two parts -- within 1e-13 (1 + S_i), the
    figure of tests/test_gpu_rollout_vjp.py, S_i from the reference sweep on the 8-step logs; bad parameter lanes
    (lb > ub, alpha NaN, alpha 0) fail every step and leave their wave neighbours bit-identical."""
    T, dt = 8, 1e-2
    flt = make_filter(hip, name)
    p = Plant(flt, RK4)
    b, g = batch(name, T), weights(name, T)
    b0 = dict(batch(name, 1), v=None)
    fw0 = dict(xlog=np.zeros((0, 2, NB)), ulog=np.zeros((0, 1, NB)), rclog=np.zeros((0, NB), dtype=np.int32))
    got = par.backward(p, fw0, b0, 0, dt, g[0], g[1])
    assert np.array_equal(got["gx0"], g[0]) and np.array_equal(got["guact0"], g[1])
    for k in ("gk", "gK", "galpha", "glb", "gub", "nskip"):
        assert np.all(got[k] == 0), k
    s = pol._state(b0, 0, NB)
    flt.rollout_plant(0, dt, RK4, s["x"], view(b0["k"], NB), s["uact"], s["relax"], s["nfail"], alpha=view(b0["alpha"], NB))
    torch.cuda.synchronize()
    assert np.array_equal(s["x"].cpu().numpy(), b0["x0"]) and np.array_equal(s["uact"].cpu().numpy(), b0["uprev"])
    lib = hip.load()
    assert lib.asif_hip_rollout_plant_batch(flt.handle, 0, 0, T, dt, RK4, *([None] * 14)) == 0
    assert lib.asif_hip_rollout_plant_vjp_batch(flt.handle, 0, 0, T, dt, RK4, *([None] * 23)) == 0

    whole = par.forward(p, b, T, dt)
    wg = par.backward(p, whole, b, T, dt, *g)
    first = par.forward(p, dict(b, v=b["v"][:3]), 3, dt)
    second = par.forward(p, dict(b, x0=first["xT"], uprev=first["uactT"], v=b["v"][3:]), 5, dt)
    for k in ("xT", "uactT"):
        assert np.array_equal(second[k], whole[k]), k
    for k in ("xlog", "ulog", "rclog"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    g2 = par.backward(p, second, dict(b, v=b["v"][3:]), 5, dt, g[0], g[1], g[2][3:], g[3][3:])
    g1 = par.backward(p, first, dict(b, v=b["v"][:3]), 3, dt, g2["gx0"], g2["guact0"], g[2][:3], g[3][:3])
    assert np.array_equal(g1["gx0"], wg["gx0"]) and np.array_equal(g1["guact0"], wg["guact0"])
    assert np.array_equal(np.concatenate([g1["gv"], g2["gv"]]), wg["gv"])
    S = reference(name, whole, b, dt, 0, *g)["S"]
    for k in ("gk", "gK", "galpha", "glb", "gub"):
        gap = np.abs((g1[k] + g2[k]) - wg[k]) / (1.0 + S)
        print(f"{name} {k}, one sweep against two: max gap {gap.max():.3e} of 1 + S (bound 1e-13)")
        assert gap.max() <= 1e-13, (k, float(gap.max()))

    bad = dict(b, alpha=b["alpha"].copy(), lb=b["lb"].copy(), ub=b["ub"].copy())
    swapped, nan, zero = np.array([3, 64, 130, 700]), np.array([5, 63, 131, 1500]), np.array([0, 65, 255, 2047])
    bad["lb"][0, swapped], bad["ub"][0, swapped] = b["ub"][0, swapped], b["lb"][0, swapped]
    bad["alpha"][nan] = np.nan
    bad["alpha"][zero] = 0.0
    hit = np.zeros(NB, dtype=bool)
    hit[np.concatenate([swapped, nan, zero])] = True
    fw = par.forward(p, bad, T, dt)
    assert np.all(fw["rclog"][:, hit] == -1) and np.all(fw["nfail"][hit] == T)
    for k, a in whole.items():
        assert np.array_equal(fw[k][..., ~hit], a[..., ~hit]), k
    gb = par.backward(p, fw, bad, T, dt, *g)
    for k in GRADS:
        assert np.array_equal(gb[k][..., ~hit], wg[k][..., ~hit]), k
    assert np.all(gb["nskip"] == 0)
    flt.close()


@pytest.mark.parametrize("name", MODELS)
def test_refusals_leave_everything_as_it_was(hip, name):
    """The refusals of tests/test_gpu_rollout_params.py, walked through both plant entries under RK4 (and the handle and
    integrator checks under Euler too): an unknown integrator is EINVAL; a handle of another variant (implicit,
    realizable, robust-data), of the two-input model or in a solver mode the light kernel does not implement is
    EUNSUPPORTED, forward and backward; a missing required pointer, gK without K, gv without v, a parameter gradient
    without its parameter, ld < B, T < 0, B < 0 are EINVAL; every optional argument may be absent.  Afterwards the handle
    still agrees with the reference, and all six existing rollout entries, on a fresh handle, give what they gave
    before any call of the new ones."""
    lib = hip.load()
    n, T = 8, 2
    T0, dt0 = 8, 1e-2
    bp, gp_ = batch(name, T0), weights(name, T0)
    b0, g0 = pol.batch(T0), pol.weights(T0)
    bc = pol.batch(T0, hasK=False, hasV=False)

    def existing():
        out = []
        di = make_filter(hip, "di")  # asif_hip_rollout_batch / _vjp_batch are the double integrator's
        fc = pol.forward_constant(di, bc, T0, dt0)
        res = [torch.empty((r, NB), dtype=torch.float64, device=DEV) for r in (2, 1, 1)]
        nskip = torch.empty(NB, dtype=torch.int32, device=DEV)
        di.rollout_vjp(T0, dt0, view(fc["xlog"], NB), view(fc["ulog"], NB), view(fc["rclog"], NB, torch.int32),
                       view(bc["k"], NB), view(g0[0], NB), *res, nskip, guactT=view(g0[1], NB), gxlog=view(g0[2], NB),
                       gulog=view(g0[3], NB))
        torch.cuda.synchronize()
        out += list(fc.values()) + [t.cpu().numpy() for t in res] + [nskip.cpu().numpy()]
        di.close()
        flt = make_filter(hip, name)
        bpol = {k: bp[k] for k in ("x0", "k", "K", "v", "uprev")}
        fp = pol.forward(flt, bpol, T0, dt0)
        out += list(fp.values()) + list(pol.backward(flt, fp, bpol, T0, dt0, *gp_).values())
        fq = par.forward(flt, bp, T0, dt0)
        out += list(fq.values()) + list(par.backward(flt, fq, bp, T0, dt0, *gp_).values())
        flt.close()
        return out
    before = existing()

    buf = [torch.ones((T * 2, n), dtype=torch.float64, device=DEV) for _ in range(26)]
    rclog = torch.ones((T, n), dtype=torch.int32, device=DEV)
    ints = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = [C.c_void_p(t.data_ptr()) for t in buf]
    prc, pin = C.c_void_p(rclog.data_ptr()), C.c_void_p(ints.data_ptr())

    def fwd(flt, nb=n, ld=n, steps=T, plant=RK4, **null):
        a = dict(x=p[0], K=p[1], k=p[2], v=p[3], alpha=p[17], lb=p[18], ub=p[19], uact=p[4], relax=p[5], nfail=pin,
                 xlog=p[6], ulog=p[7], rclog=prc)
        a.update(null)
        return lib.asif_hip_rollout_plant_batch(flt.handle, nb, ld, steps, 1e-3, plant, *a.values(), None)

    def bwd(flt, nb=n, ld=n, steps=T, plant=RK4, **null):
        a = dict(xlog=p[6], ulog=p[7], rclog=prc, K=p[1], k=p[2], v=p[3], alpha=p[17], lb=p[18], ub=p[19], gxT=p[8],
                 guactT=p[9], gxlog=p[10], gulog=p[11], gx0=p[12], gK=p[13], gk=p[14], gv=p[15], galpha=p[20], glb=p[21],
                 gub=p[22], guact0=p[16], nskip=pin)
        a.update(null)
        return lib.asif_hip_rollout_plant_vjp_batch(flt.handle, nb, ld, steps, 1e-3, plant, *a.values(), None)

    others = [hip.Filter(*hip.CONFIGS[3][:2]), hip.Filter(*hip.CONFIGS[11][:2]),  # implicit; the two-input model
              hip.RealizableFilter(workloads.load_kernel()), hip.RobustDataFilter(workloads.load_halfplanes()),
              make_filter(hip, name, polish=1), make_filter(hip, name, polish=0), make_filter(hip, name, lanes_per_qp=4)]
    for other in others:
        for plant in (EULER, RK4):
            assert fwd(other, plant=plant) == EUNSUPPORTED and bwd(other, plant=plant) == EUNSUPPORTED
        other.close()
    pre = make_filter(hip, name, polish=1, presolve=1)  # presolve: the light kernel forwards; the sweep wants polish == 2
    assert fwd(pre) == 0 and bwd(pre) == EUNSUPPORTED
    pre.close()
    pre = make_filter(hip, name, presolve=1)
    assert fwd(pre) == 0 and bwd(pre) == 0
    torch.cuda.synchronize()
    pre.close()

    flt = make_filter(hip, name)
    for plant in (2, -1, 7):
        assert fwd(flt, plant=plant) == EINVAL and bwd(flt, plant=plant) == EINVAL
        assert fwd(flt, plant=plant, nb=0) == EINVAL and bwd(flt, plant=plant, nb=0) == EINVAL
    for k in ("x", "k", "uact", "relax", "nfail"):
        assert fwd(flt, **{k: None}) == EINVAL, k
    for k in ("xlog", "ulog", "rclog", "k", "gxT", "gx0", "gk", "guact0", "nskip"):
        assert bwd(flt, **{k: None}) == EINVAL, k
    assert bwd(flt, K=None) == EINVAL and bwd(flt, v=None) == EINVAL  # gK without K, gv without v
    for k in par.PARAMS:  # a gradient asked for a parameter that was not given
        assert bwd(flt, **{k: None}) == EINVAL, k
        assert bwd(flt, **{k: None, "g" + k: None}) == 0, k
    for call in (fwd, bwd):
        assert call(flt, ld=n - 1) == EINVAL and call(flt, steps=-1) == EINVAL and call(flt, nb=-1) == EINVAL
        assert call(flt, nb=0) == 0 and call(flt) == 0 and call(flt, plant=EULER) == 0
    assert fwd(flt, K=None, v=None, alpha=None, lb=None, ub=None, xlog=None, ulog=None, rclog=None) == 0
    assert fwd(flt, steps=0) == 0
    assert bwd(flt, guactT=None, gxlog=None, gulog=None, gK=None, gv=None, galpha=None, glb=None, gub=None) == 0
    assert bwd(flt, K=None, gK=None, v=None, gv=None, alpha=None, galpha=None, lb=None, glb=None, ub=None, gub=None) == 0
    assert bwd(flt, steps=0, xlog=None, ulog=None, rclog=None) == 0
    torch.cuda.synchronize()

    # still usable: a forward and a backward pass under RK4 agree with the reference
    Tn, dtn, m = 4, 1e-2, 64
    b, g = batch(name, Tn, m), weights(name, Tn, m)
    fw = par.forward(Plant(flt, RK4), b, Tn, dtn)
    par.check_parity(par.backward(Plant(flt, RK4), fw, b, Tn, dtn, *g), reference(name, fw, b, dtn, 0, *g), m,
                     f"{name} after the refusals")
    flt.close()

    for a, c in zip(before, existing()):
        assert (a is None and c is None) or np.array_equal(a, c)


def test_torch_layers_take_the_integrator(hip):
    """ParamRolloutLayer / PolicyRolloutLayer with integrator="rk4": the direct entries' outputs and gradients bit for
    bit; with the default argument they still equal the Euler entries; an unknown name raises."""
    from asif_amd.torch_layer import ParamRolloutLayer, PolicyRolloutLayer
    T, dt = 8, 1e-2
    b, gn = batch("cp", T), weights("cp", T)
    g = tuple(torch.from_numpy(a).to(DEV) for a in gn)
    names = (("gx0", "x0"), ("gk", "k"), ("gK", "K"), ("gv", "v"), ("guact0", "uprev"), ("galpha", "alpha"), ("glb", "lb"),
             ("gub", "ub"))
    for integrator, wrap in (("rk4", lambda f: Plant(f, RK4)), (None, lambda f: f)):
        kw = {} if integrator is None else dict(integrator=integrator)
        layer = ParamRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt, **kw)
        lv = cpt._leaves(b)
        outs = layer(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"], alpha=lv["alpha"], lb=lv["lb"],
                     ub=lv["ub"])
        fw = par.forward(wrap(layer.filter), b, T, dt)
        for o, k in zip(outs, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
            assert np.array_equal(o.detach().cpu().numpy(), fw[k]), (integrator, k)
        cpt._segment_loss(outs, g).backward()
        torch.cuda.synchronize()
        want = par.backward(wrap(layer.filter), fw, b, T, dt, *gn)
        for name, leaf in names:
            assert np.array_equal(lv[leaf].grad.cpu().numpy(), want[name]), (integrator, name)
    bp = batch("cp", T, params=())
    player = PolicyRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt, integrator="rk4")
    lv = cpt._leaves(bp)
    outs = player(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"])
    fwp = par.forward(Plant(player.filter, RK4), bp, T, dt)
    for o, k in zip(outs, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
        assert np.array_equal(o.detach().cpu().numpy(), fwp[k]), k
    cpt._segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    wantp = par.backward(Plant(player.filter, RK4), fwp, bp, T, dt, *gn)
    for name, leaf in names[:5]:
        assert np.array_equal(lv[leaf].grad.cpu().numpy(), wantp[name]), name
    with pytest.raises(ValueError):
        ParamRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt, integrator="heun")


def test_gradcheck_rk4_on_kink_free_instances(hip):
    """torch.autograd.gradcheck on 8 pendulum instances x 4 RK4 steps, chosen as tests/test_gpu_cart_pendulum.py chooses
    them: working sets and return codes unchanged in the reference under +-1e-5 in every input."""
    from asif_amd.torch_layer import ParamRolloutLayer
    T, dt, step = 4, 1e-2, 1e-5
    b = batch("cp", T)
    opt = options("cp")
    run = lambda c: ref.forward(cart_pendulum_ref, c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt, c["alpha"],
                                c["lb"], c["ub"])
    base = run(b)
    stable = np.ones(NB, dtype=bool)
    for name, a in b.items():
        flat = a.reshape(-1, NB)
        for row in range(flat.shape[0]):
            for sign in (1.0, -1.0):
                moved = flat.copy()
                moved[row] += sign * step
                q = run(dict(b, **{name: moved.reshape(a.shape)}))
                stable &= ((q["wid"] == base["wid"]) & (q["rclog"] == base["rclog"])).all(axis=0)
    wid = base["wid"]
    failed = (wid == -2).any(axis=0)
    fam = [failed, ((wid >= 0) & (wid < 4)).any(axis=0) & ~failed, (wid >= 4).any(axis=0) & ~failed, (wid == -1).all(axis=0)]
    pick = np.concatenate([np.flatnonzero(stable & f)[:2] for f in fam])
    assert len(pick) == 8
    layer = ParamRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt, integrator="rk4")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[..., pick])).to(DEV).requires_grad_()
    args = tuple(t(b[k]) for k in ("x0", "k", "K", "v", "uprev", "alpha", "lb", "ub"))
    fn = lambda x0, k, K, v, up, al, lb, ub: layer(x0, k, K=K, v=v, uact_prev=up, alpha=al, lb=lb, ub=ub)[:4]
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-3, nondet_tol=0.0)
