"""Class ASIF on the synthetic cart-driven pendulum (ASIF_HIP_MODEL_CART_PENDULUM) on the device: the filter, its rows and
its vector-Jacobian product, the fused rollout under an affine policy with the parameters per instance and its adjoint,
and the torch layer -- against the numpy reference of tests/cart_pendulum_ref.py (itself checked against finite differences
in tests/test_cart_pendulum_ref_host.py).  The oracle has no such model.

Device and numpy evaluate sin / cos with different code: they may differ in the last bits.  A return code is therefore
compared exactly except where the reference's own feasibility test sits within 1e-12 (relative) of its threshold; such
instances are counted, printed and capped at 0.1 %.  Backward passes run the numpy sweep on the DEVICE's own logs; bound per
gradient entry 1e-9 (1 + S_i) max(1, 1 / a_min,i) as tests/test_gpu_rollout_params.py, no instance left out.
The buffers (padded, sentinels) and the launch helpers are those of tests/test_gpu_rollout_policy.py / _params.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cart_pendulum_ref as ref
import test_cart_pendulum_ref_host as host
import test_gpu_rollout_params as par
import test_gpu_rollout_policy as pol

pytestmark = pytest.mark.gpu

DEV, NB, SENTINEL = pol.DEV, pol.NB, pol.SENTINEL
GRADS = par.GRADS
view, padded = pol.view, pol.padded
SHAPES = host.SHAPES
EUNSUPPORTED = -3


def make_filter(hip, keep=0, **solver):
    od = hip.default_options(hip.MODEL_CART_PENDULUM, hip.EXPLICIT)
    od.npSSmax = keep
    return hip.Filter(hip.MODEL_CART_PENDULUM, hip.EXPLICIT, options=od,
                      solver=hip.default_solver(**solver) if solver else None)


def batch(T, n=NB, hasK=True, hasV=True, params=par.PARAMS):
    b = host.inputs(T, n)
    if not hasK:
        b["K"] = None
    if not hasV:
        b["v"] = None
    for p in par.PARAMS:
        if p not in params:
            b[p] = None
    return b


def weights(T, n=NB):
    return host.weights(T, n)


def reference(fw, b, dt, keep, gxT, guactT=None, gxlog=None, gulog=None):
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], b["k"], b["K"], b["v"], dt, ref.options(keep), gxT, guactT,
                       gxlog, gulog, b["alpha"], b["lb"], b["ub"])


def rc_agrees(got_rc, s, what, budget):
    """got_rc against the reference's verdict; a difference is allowed only within 1e-12 of the reference's threshold.
    Returns the mask of instances to compare further; budget: a one-element list that collects the excepted count."""
    want = np.where(s["ok"], 1, -1)
    diff = got_rc != want
    assert np.all(s["margin"][diff] < 1e-12), f"{what}: {int((diff & (s['margin'] >= 1e-12)).sum())} rc differ away from the threshold"
    budget[0] += int(diff.sum())
    return ~diff


def test_default_options_and_dims(hip):
    o = hip.default_options(hip.MODEL_CART_PENDULUM, hip.EXPLICIT)
    want = ref.options()
    assert (o.lb[0], o.ub[0], o.relaxLb, o.relaxCost) == (want["lb"], want["ub"], want["relaxLb"], want["relaxCost"])
    for keep, nc in ((0, 4), (2, 2), (7, 4)):
        flt = make_filter(hip, keep)
        d = flt.dims
        assert (d.nx, d.nu, d.npSS, d.nv, d.nc, d.nrelax, d.ndiag) == (2, 1, 4, 2, nc, 1, 4)
        flt.close()
    for variant in (hip.IMPLICIT, hip.IMPLICIT_TB, hip.ROBUST, hip.IMPLICIT_RB):  # explicit handles only
        with pytest.raises(hip.AsifHipError):
            hip.Filter(hip.MODEL_CART_PENDULUM, variant, options=o)


@pytest.mark.parametrize("keep", [0, 2])
def test_filter_and_rows_on_2048_states(hip, keep):
    """asif_hip_filter_batch: u within 1e-9 (1 + |u|) of the reference projection, rc equal but for the threshold rule,
    a failed instance keeps what uact held; asif_hip_assemble_batch: every row entry within 1e-12 (1 + |entry|)."""
    b = batch(1)
    opt = ref.options(keep)
    s = ref.filter_step(b["x0"], b["k"][0], opt["keep"], *ref.lane_params(opt, NB))
    flt = make_filter(hip, keep)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    uact, relax = t(b["uprev"]), torch.zeros((1, NB), dtype=torch.float64, device=DEV)
    rc = torch.zeros(NB, dtype=torch.int32, device=DEV)
    flt.filter(t(b["x0"]), t(b["k"]), uact, relax, rc)
    nc = opt["keep"]
    A, bb = torch.zeros((nc * 2, NB), dtype=torch.float64, device=DEV), torch.zeros((nc, NB), dtype=torch.float64, device=DEV)
    code, diag = torch.zeros(NB, dtype=torch.int32, device=DEV), torch.zeros((4, NB), dtype=torch.float64, device=DEV)
    flt.assemble(t(b["x0"]), A, bb, code, diag)
    torch.cuda.synchronize()
    budget = [0]
    same = rc_agrees(rc.cpu().numpy(), s, f"keep={keep}", budget)
    print(f"keep={keep}: {budget[0]} of {NB} return codes excepted (within 1e-12 of the threshold)")
    assert budget[0] <= NB // 1000
    want = np.where(s["ok"], s["u"], b["uprev"][0])
    gap = np.abs(uact.cpu().numpy()[0] - want) / (1.0 + np.abs(want))
    print(f"keep={keep}: max |u - ref| / (1 + |u|) = {gap[same].max():.3e} (bound 1e-9); "
          f"{int(s['ok'].sum())} solved, {int((~s['ok']).sum())} failed")
    assert gap[same].max() <= 1e-9
    assert s["ok"].sum() > 500 and (~s["ok"]).sum() > 100
    assert np.array_equal(relax.cpu().numpy()[0][same & s["ok"]], np.full(int((same & s["ok"]).sum()), opt["relaxLb"]))
    wA, wb, which = ref.rows(b["x0"], nc)
    got_which = diag.cpu().numpy()[:nc]
    order_same = np.all(got_which == which, axis=0)  # two h within the last bits of one another may swap rows
    print(f"keep={keep}: {int((~order_same).sum())} instances with another row order")
    assert (~order_same).sum() <= NB // 1000
    for name, got, w in (("A", A.cpu().numpy(), wA), ("b", bb.cpu().numpy(), wb)):
        gap = np.abs(got - w) / (1.0 + np.abs(w))
        print(f"keep={keep} rows {name}: max gap {gap[:, order_same].max():.3e} (bound 1e-12)")
        assert gap[:, order_same].max() <= 1e-12
    assert np.all(code.cpu().numpy() == 1)
    flt.close()


@pytest.mark.parametrize("lie", [False, True])
@pytest.mark.parametrize("keep", [0, 2])
def test_filter_vjp(hip, lie, keep):
    """asif_hip_filter_vjp_batch with the model's own Lie derivatives and with caller-supplied ones against the
    reference's one-step adjoint: 1e-9 (1 + |ref|) max(1, 1 / sigma_min(G_W)), the bound of tests/test_gpu_explicit_vjp.py."""
    b = batch(1)
    opt = ref.options(keep)
    nc = opt["keep"]
    rng = np.random.default_rng(77)
    gbar = rng.normal(0, 1, (1, NB))
    lies = (rng.normal(0, 1, (nc, NB)), rng.normal(0, 1, (nc, NB))) if lie else None
    want = ref.filter_vjp(b["x0"], b["k"][0], gbar[0], opt, lies)
    flt = make_filter(hip, keep)
    ld = NB + 64
    out = dict(gudes=padded(np.full((1, NB), SENTINEL), ld))
    if lie:
        out.update(glfh=padded(np.full((nc, NB), SENTINEL), ld), glgh=padded(np.full((nc, NB), SENTINEL), ld),
                   gx=padded(np.full((2, NB), SENTINEL), ld))
    rc = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    o = lambda k: out[k][1] if k in out else None
    flt.filter_vjp(view(b["x0"], ld), view(b["k"], ld), view(gbar, ld), o("gudes"), rc, view(lies[0], ld) if lie else None,
                   view(lies[1], ld) if lie else None, o("glfh"), o("glgh"), o("gx"))
    torch.cuda.synchronize()
    got_rc = rc.cpu().numpy()
    assert np.all(got_rc[NB:] == -77)
    budget = [0]
    same = rc_agrees(got_rc[:NB], dict(ok=want["rc"] == 1, margin=want["margin"]), f"lie={lie}", budget)
    assert budget[0] <= NB // 1000
    scale = np.maximum(1.0, 1.0 / want["smin"])
    for k, (buf, _) in out.items():
        g = buf.cpu().numpy()
        assert np.all(g[:, NB:] == SENTINEL), f"{k}: slots >= B written"
        gap = np.abs(g[:, :NB] - want[k]) / ((1.0 + np.abs(want[k])) * scale[None, :])
        print(f"lie={lie} keep={keep} {k}: max scaled gap {gap[:, same].max():.3e} (bound 1e-9)")
        assert gap[:, same].max() <= 1e-9, k
        assert np.all(g[:, :NB][:, same & (want["rc"] != 1)] == 0.0), f"{k}: a failed instance holds a gradient"
    wid = want["wid"][want["rc"] == 1]
    assert (wid < 0).sum() > 100 and ((wid >= 0) & (wid < 4)).sum() > 100 and (wid >= 4).sum() > 100
    flt.close()


def device_forward(flt, b, T, dt, ld=None):
    return par.forward(flt, b, T, dt, ld)


def device_backward(flt, fw, b, T, dt, g, ld=None, **kw):
    return par.backward(flt, fw, b, T, dt, *g, ld=ld, **kw)


@pytest.mark.parametrize("keep", [0, 2])
@pytest.mark.parametrize("T,dt", SHAPES)
def test_rollout_forward_step_by_step_on_the_device_logs(hip, T, dt, keep):
    """On xlog[t]: rclog[t] by the threshold rule, ulog[t] within 1e-9 (1 + |u|) of the reference, x_{t+1} within
    1e-14 (1 + |x|) of the numpy Euler step of (xlog[t], ulog[t]), nfail counts rclog < 0, relax is alpha_i where a step
    solved, and ulog[t] against asif_hip_filter_batch on (xlog[t], uDes_t) within 1e-12 (1 + |u|) (reported: bit for bit
    or not)."""
    flt = make_filter(hip, keep)
    b = batch(T)
    fw = device_forward(flt, b, T, dt)
    opt = ref.options(keep)
    lane = ref.lane_params(opt, NB, b["alpha"], b["lb"], b["ub"])
    assert np.array_equal(fw["xlog"][0], b["x0"])
    budget, worst_u, worst_x = [0], 0.0, 0.0
    prev = b["uprev"][0]
    udes_all = np.zeros((T, NB))
    for t in range(T):
        xt, ut = fw["xlog"][t], fw["ulog"][t, 0]
        udes_all[t] = ref.policy(b["k"], b["K"], b["v"][t], xt)
        s = ref.filter_step(xt, udes_all[t], opt["keep"], *lane)
        same = rc_agrees(fw["rclog"][t], s, f"step {t}", budget)
        want = np.where(fw["rclog"][t] == 1, s["u"], prev)
        worst_u = max(worst_u, float((np.abs(ut - want) / (1.0 + np.abs(want)))[same].max()))
        assert np.array_equal(ut[fw["rclog"][t] < 0], prev[fw["rclog"][t] < 0]), f"step {t}: a failed step moved u"
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        step = ref.plant_step(xt, ut, dt)
        worst_x = max(worst_x, float((np.abs(nxt - step) / (1.0 + np.abs(step))).max()))
        prev = ut
    print(f"T={T} dt={dt} keep={keep}: {budget[0]} of {T * NB} return codes excepted; max u gap {worst_u:.3e} (bound 1e-9); "
          f"max Euler gap {worst_x:.3e} (bound 1e-14)")
    assert budget[0] <= (T * NB) // 1000
    assert worst_u <= 1e-9 and worst_x <= 1e-14
    assert np.array_equal(fw["uactT"][0], fw["ulog"][-1, 0])
    assert np.array_equal(fw["nfail"], (fw["rclog"] < 0).sum(axis=0))
    some = (fw["rclog"] > 0).any(axis=0)
    assert np.array_equal(fw["relax"][0][some], b["alpha"][some])
    failed = fw["rclog"] < 0
    assert failed.any() and (~failed).any()
    if T > 1:
        assert (failed.any(axis=0) & (~failed).any(axis=0)).any()

    # the filter entry on the logged states: per-instance parameters are the handle's here, so a second rollout with them
    bh = batch(T, params=())
    fh = device_forward(flt, bh, T, dt)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    worst, bitwise = 0.0, True
    prev = bh["uprev"][0]
    for t in range(T):
        xt = fh["xlog"][t]
        udes = ref.policy(bh["k"], bh["K"], bh["v"][t], xt)
        uact, relax = t_(prev[None, :]), torch.zeros((1, NB), dtype=torch.float64, device=DEV)
        rc = torch.zeros(NB, dtype=torch.int32, device=DEV)
        flt.filter(t_(xt), t_(udes[None, :]), uact, relax, rc)
        torch.cuda.synchronize()
        u = uact.cpu().numpy()[0]
        assert np.array_equal(rc.cpu().numpy(), fh["rclog"][t]), f"step {t}: filter entry and rollout disagree on rc"
        worst = max(worst, float((np.abs(u - fh["ulog"][t, 0]) / (1.0 + np.abs(u))).max()))
        bitwise &= np.array_equal(u, fh["ulog"][t, 0])
        prev = fh["ulog"][t, 0]
    print(f"T={T} dt={dt} keep={keep}: ulog against asif_hip_filter_batch: max gap {worst:.3e} (bound 1e-12), "
          f"bit for bit: {bitwise}")
    assert worst <= 1e-12
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [(1, 1e-3, NB, NB, 0), (8, 1e-2, NB, NB, 0), (40, 1e-3, NB, NB, 0),
                                            (8, 1e-2, NB, NB, 2), (8, 1e-2, 65, 192, 0), (1, 1e-3, 1, 1, 0)])
def test_device_sweep_matches_reference_on_device_logs(hip, T, dt, n, ld, keep):
    """Every gradient within 1e-9 (1 + S) max(1, 1 / amin) of the numpy sweep on the device's logs, nskip 0, padding and
    sentinels untouched, every slot i < B written."""
    flt = make_filter(hip, keep)
    b = batch(T, n)
    fw = device_forward(flt, b, T, dt, ld)
    g = weights(T, n)
    got = device_backward(flt, fw, b, T, dt, g, ld)
    adj = reference(fw, b, dt, keep, *g)
    par.check_parity(got, adj, n, f"T={T} dt={dt} B={n} ld={ld} keep={keep}")
    for k in GRADS:
        assert np.all(got[k][..., n:] == SENTINEL), f"{k}: slots >= B written"
        assert not np.any(got[k][..., :n] == SENTINEL), f"{k}: a slot < B not written"
    assert np.all(got["nskip"][n:] == -77)
    if (T, n, keep) == (8, NB, 0):
        assert adj["nrow"] >= 100 and adj["nlb"] >= 100 and adj["nub"] >= 100, (adj["nrow"], adj["nlb"], adj["nub"])
    flt.close()


def test_every_optional_input_and_gradient(hip):
    """guactT, gxlog, gulog, K, v and each parameter present and absent, each on its own forward pass."""
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    g = weights(T)
    for hasK, hasV, params in ((False, True, par.PARAMS), (True, False, ("alpha",)), (True, True, ("lb",)),
                               (True, True, ("ub",)), (False, False, ())):
        b = batch(T, hasK=hasK, hasV=hasV, params=params)
        fw = device_forward(flt, b, T, dt)
        par.check_parity(device_backward(flt, fw, b, T, dt, g), reference(fw, b, dt, 0, *g), NB,
                         f"K={hasK} v={hasV} params={params}")
    b = batch(T)
    fw = device_forward(flt, b, T, dt)
    for gg, what in (((g[0], None, None, None), "gxT alone"), ((g[0], g[1], None, None), "no log gradients"),
                     ((g[0], None, g[2], None), "gxlog"), ((g[0], None, None, g[3]), "gulog")):
        par.check_parity(device_backward(flt, fw, b, T, dt, gg), reference(fw, b, dt, 0, *gg), NB, what)
    full = device_backward(flt, fw, b, T, dt, g)
    got = device_backward(flt, fw, b, T, dt, g, gK=False, gv=False, gpar=False)
    for k in ("gx0", "gk", "guact0", "nskip"):
        assert np.array_equal(got[k], full[k]), k
    flt.close()


def test_identities(hip):
    """Parameters NULL, and filled with the handle's values: the policy entries bit for bit; K = v = NULL backward across
    the WANTP instantiations bit for bit; T = 0 the identity; B = 0 returns OK."""
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    g = weights(T)
    b = batch(T, params=())
    want = pol.forward(flt, b, T, dt)
    wantg = pol.backward(flt, want, b, T, dt, *g)
    o = ref.options()
    filled = dict(b, alpha=np.full(NB, o["relaxLb"]), lb=np.full((1, NB), o["lb"]), ub=np.full((1, NB), o["ub"]))
    for name, bb in (("NULL", b), ("the handle's values", filled)):
        got = device_forward(flt, bb, T, dt)
        for k, a in want.items():
            assert np.array_equal(got[k], a), (name, k)
        gotg = device_backward(flt, got, bb, T, dt, g)
        for k, a in wantg.items():
            assert np.array_equal(gotg[k], a), (name, k)

    bn = dict(filled, K=None, v=None)
    fw = device_forward(flt, bn, T, dt)
    withp = device_backward(flt, fw, bn, T, dt, g)
    without = device_backward(flt, fw, bn, T, dt, g, gpar=False)
    for k in ("gx0", "gk", "guact0", "nskip"):
        assert np.array_equal(withp[k], without[k]), k

    b0 = dict(batch(1), v=None)
    fw0 = dict(xlog=np.zeros((0, 2, NB)), ulog=np.zeros((0, 1, NB)), rclog=np.zeros((0, NB), dtype=np.int32))
    g0 = weights(1)
    got = device_backward(flt, fw0, b0, 0, dt, (g0[0], g0[1]))
    assert np.array_equal(got["gx0"], g0[0]) and np.array_equal(got["guact0"], g0[1])
    for k in ("gk", "gK", "galpha", "glb", "gub", "nskip"):
        assert np.all(got[k] == 0), k
    s = pol._state(b0, 0, NB)
    flt.rollout_params(0, dt, s["x"], view(b0["k"], NB), s["uact"], s["relax"], s["nfail"], alpha=view(b0["alpha"], NB))
    torch.cuda.synchronize()
    assert np.array_equal(s["x"].cpu().numpy(), b0["x0"]) and np.array_equal(s["uact"].cpu().numpy(), b0["uprev"])

    lib = hip.load()
    assert lib.asif_hip_rollout_params_batch(flt.handle, 0, 0, T, dt, *([None] * 14)) == 0
    assert lib.asif_hip_rollout_params_vjp_batch(flt.handle, 0, 0, T, dt, *([None] * 23)) == 0
    assert lib.asif_hip_rollout_policy_batch(flt.handle, 0, 0, T, dt, *([None] * 11)) == 0
    assert lib.asif_hip_rollout_policy_vjp_batch(flt.handle, 0, 0, T, dt, *([None] * 17)) == 0
    flt.close()


def test_refusals_and_bad_parameters(hip):
    """asif_hip_rollout_batch / asif_hip_rollout_vjp_batch stay the double integrator's; the sweeps want polish == 2; bad
    parameter data (lb > ub, alpha NaN, alpha 0, a NaN bound) fails every step of its instance and leaves the others
    bit-identical.  (An upper bound of +inf is not bad data to these kernels: qp_lane.hpp takes an infinite bound as
    one-sided, on this model as on the double integrator.)"""
    lib = hip.load()
    n, T, dt = 8, 2, 1e-3
    buf = [torch.ones((T * 2, n), dtype=torch.float64, device=DEV) for _ in range(14)]
    ints = torch.ones((T, n), dtype=torch.int32, device=DEV)
    p = [C.c_void_p(t.data_ptr()) for t in buf]
    pi = C.c_void_p(ints.data_ptr())
    flt = make_filter(hip)
    assert lib.asif_hip_rollout_batch(flt.handle, n, n, T, dt, p[0], p[1], p[2], p[3], pi, p[4], p[5], pi, None) == EUNSUPPORTED
    assert lib.asif_hip_rollout_vjp_batch(flt.handle, n, n, T, dt, p[0], p[1], pi, p[2], p[3], p[4], p[5], p[6], p[7], p[8],
                                          p[9], pi, None) == EUNSUPPORTED
    flt.close()

    Tn, dtn, m = 4, 1e-2, 64
    b, g = batch(Tn, m), weights(Tn, m)
    for solver, fwd_ok in ((dict(polish=1, presolve=1), True), (dict(polish=1), False), (dict(polish=0), False),
                           (dict(lanes_per_qp=4), False)):
        other = make_filter(hip, **solver)
        if fwd_ok:
            fw = device_forward(other, b, Tn, dtn)
        else:
            with pytest.raises(hip.AsifHipError, match="-3"):
                device_forward(other, b, Tn, dtn)
            fw = dict(xlog=np.zeros((Tn, 2, m)), ulog=np.zeros((Tn, 1, m)), rclog=np.ones((Tn, m), dtype=np.int32))
        with pytest.raises(hip.AsifHipError, match="-3"):
            device_backward(other, fw, b, Tn, dtn, g)
        with pytest.raises(hip.AsifHipError, match="-3"):
            pol.backward(other, fw, b, Tn, dtn, *g)
        other.close()

    T, dt = 8, 1e-2
    flt = make_filter(hip)
    b, g = batch(T), weights(T)
    clean = device_forward(flt, b, T, dt)
    cleang = device_backward(flt, clean, b, T, dt, g)
    bad = dict(b, alpha=b["alpha"].copy(), lb=b["lb"].copy(), ub=b["ub"].copy())
    swapped, nan, zero, nanb = np.array([3, 64, 130, 700]), np.array([5, 63, 131, 1500]), np.array([0, 65, 255, 2047]), np.array([7, 66, 900])
    bad["lb"][0, swapped], bad["ub"][0, swapped] = b["ub"][0, swapped], b["lb"][0, swapped]
    bad["alpha"][nan] = np.nan
    bad["alpha"][zero] = 0.0
    bad["ub"][0, nanb[:2]], bad["lb"][0, nanb[2:]] = np.nan, np.nan
    hit = np.zeros(NB, dtype=bool)
    hit[np.concatenate([swapped, nan, zero, nanb])] = True
    fw = device_forward(flt, bad, T, dt)
    assert np.all(fw["rclog"][:, hit] == -1) and np.all(fw["nfail"][hit] == T)
    assert np.array_equal(fw["uactT"][0][hit], b["uprev"][0][hit])
    for k, a in clean.items():
        assert np.array_equal(fw[k][..., ~hit], a[..., ~hit]), k
    got = device_backward(flt, fw, bad, T, dt, g)
    for k in GRADS:
        assert np.array_equal(got[k][..., ~hit], cleang[k][..., ~hit]), k
    for k in ("galpha", "glb", "gub", "gk"):
        assert np.all(got[k][..., hit] == 0), k
    assert np.all(got["nskip"] == 0)
    flt.close()


def _segment_loss(outs, g):
    xT, uactT, xlog, ulog = outs[:4]
    return (xT * g[0]).sum() + (uactT * g[1]).sum() + (xlog * g[2]).sum() + (ulog * g[3]).sum()


def _leaves(b):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_()
    return {k: t(a) for k, a in b.items()}


def test_torch_layer_is_the_two_launches(hip):
    """ParamRolloutLayer(model=MODEL_CART_PENDULUM): .backward() gives the direct entry's gradients bit for bit;
    PolicyRolloutLayer and ExplicitSafetyLayer accept the model; ExplicitRolloutLayer refuses it."""
    from asif_amd.torch_layer import ExplicitRolloutLayer, ExplicitSafetyLayer, ParamRolloutLayer, PolicyRolloutLayer
    T, dt = 8, 1e-2
    layer = ParamRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt)
    b, gn = batch(T), weights(T)
    g = tuple(torch.from_numpy(a).to(DEV) for a in gn)
    lv = _leaves(b)
    outs = layer(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"], alpha=lv["alpha"], lb=lv["lb"], ub=lv["ub"])
    fw = device_forward(layer.filter, b, T, dt)
    for o, k in zip(outs, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
        assert np.array_equal(o.detach().cpu().numpy(), fw[k]), k
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    want = device_backward(layer.filter, fw, b, T, dt, gn)
    for name, leaf in (("gx0", "x0"), ("gk", "k"), ("gK", "K"), ("gv", "v"), ("guact0", "uprev"), ("galpha", "alpha"),
                       ("glb", "lb"), ("gub", "ub")):
        assert np.array_equal(lv[leaf].grad.cpu().numpy(), want[name]), name

    bp = batch(T, params=())
    player = PolicyRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt)
    lv = _leaves(bp)
    outs = player(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"])
    fwp = pol.forward(player.filter, bp, T, dt)
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    wantp = pol.backward(player.filter, fwp, bp, T, dt, *gn)
    for name, leaf in (("gx0", "x0"), ("gk", "k"), ("gK", "K"), ("gv", "v"), ("guact0", "uprev")):
        assert np.array_equal(lv[leaf].grad.cpu().numpy(), wantp[name]), name

    safety = ExplicitSafetyLayer(hip.MODEL_CART_PENDULUM)
    lv = _leaves(bp)
    uact, rc = safety(lv["x0"].detach(), lv["k"], uact_prev=lv["uprev"])
    uact.sum().backward()
    torch.cuda.synchronize()
    s = ref.filter_vjp(bp["x0"], bp["k"][0], np.ones(NB), ref.options())
    same = rc.cpu().numpy() == s["rc"]
    assert (~same).sum() <= NB // 1000
    assert np.abs(lv["k"].grad.cpu().numpy() - s["gudes"])[:, same].max() <= 1e-9

    with pytest.raises(ValueError):
        ExplicitRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt)(lv["x0"].detach(), lv["k"].detach())


def test_gradcheck_on_kink_free_instances(hip):
    """torch.autograd.gradcheck on 8 instances x 4 steps: instances whose working sets and return codes the reference
    finds unchanged under +-1e-5 in every input (ten times the check's eps), two each with a failed step, a step on a
    row, a step on a bound, and free steps only."""
    from asif_amd.torch_layer import ParamRolloutLayer
    T, dt, step = 4, 1e-2, 1e-5
    b = batch(T)
    opt = ref.options()
    run = lambda c: ref.forward(c["x0"], c["k"], c["K"], c["v"], c["uprev"], T, dt, opt, c["alpha"], c["lb"], c["ub"])
    base = run(b)
    stable = np.ones(NB, dtype=bool)
    for name, a in b.items():
        flat = a.reshape(-1, NB)
        for row in range(flat.shape[0]):
            for sign in (1.0, -1.0):
                moved = flat.copy()
                moved[row] += sign * step
                p = run(dict(b, **{name: moved.reshape(a.shape)}))
                stable &= ((p["wid"] == base["wid"]) & (p["rclog"] == base["rclog"])).all(axis=0)
    wid = base["wid"]
    fam = [(wid == -2).any(axis=0), ((wid >= 0) & (wid < 4)).any(axis=0) & ~(wid == -2).any(axis=0),
           (wid >= 4).any(axis=0) & ~(wid == -2).any(axis=0), (wid == -1).all(axis=0)]
    pick = np.concatenate([np.flatnonzero(stable & f)[:2] for f in fam])
    print(f"{int(stable.sum())} of {NB} instances kink-free within {step}; picked {pick.tolist()}")
    assert len(pick) == 8
    layer = ParamRolloutLayer(hip.MODEL_CART_PENDULUM, T=T, dt=dt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[..., pick])).to(DEV).requires_grad_()
    args = tuple(t(b[k]) for k in ("x0", "k", "K", "v", "uprev", "alpha", "lb", "ub"))
    fn = lambda x0, k, K, v, up, al, lb, ub: layer(x0, k, K=K, v=v, uact_prev=up, alpha=al, lb=lb, ub=ub)[:4]
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-3, nondet_tol=0.0)
