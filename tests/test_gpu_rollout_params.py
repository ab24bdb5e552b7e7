"""asif_hip_rollout_params_batch / asif_hip_rollout_params_vjp_batch (asif_amd/csrc/k_rollout_policy.hip, PARAMS) and the torch
layer on top of them: the fused explicit rollout under an affine policy with the barrier gain alpha_i and the input box
lb_i, ub_i per instance.

Forward: with the parameters NULL or equal to the handle's, asif_hip_rollout_policy_batch bit for bit; with them given,
every step checked on the logged states against the numpy reference of tests/rollout_params_ref.py.  Backward: the numpy
sweep of that file (itself checked against finite differences in tests/test_rollout_params_ref_host.py) run on the
DEVICE's own logs.

Parity bound per gradient entry: 1e-9 (1 + S_i) max(1, 1 / a_min,i), the bound of tests/test_gpu_rollout_policy.py with
S_i extended by the largest |h_r w_r| met along the instance's sweep.  No instance is left out.  The buffers, the batch
and the loss weights are that file's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib
import rollout_params_ref as ref
import test_gpu_rollout_policy as pol
from asif_amd import workloads

pytestmark = pytest.mark.gpu

DEV, NB, SENTINEL = pol.DEV, pol.NB, pol.SENTINEL
GRADS = ("gx0", "gK", "gk", "gv", "galpha", "glb", "gub", "guact0")
PARAMS = ("alpha", "lb", "ub")
make_filter, padded, view, weights = pol.make_filter, pol.padded, pol.view, pol.weights


def batch(T, n=NB, hasK=True, hasV=True, params=PARAMS):
    """The policy tests' batch with alpha_i in [2, 8], lb_i in [-1.5, -0.5], ub_i in [0.5, 1.5] (those named in params)."""
    b = pol.batch(T, n, hasK, hasV)
    i = np.arange(n, dtype=np.uint64)
    u = lambda j: workloads.uniform(480, i, j)
    b.update(alpha=2.0 + 6.0 * u(0), lb=(-1.5 + u(1))[None, :].copy(), ub=(0.5 + u(2))[None, :].copy())
    for p in PARAMS:
        if p not in params:
            b[p] = None
    return b


def handle_params(n):
    """Arrays filled with the default handle's own values."""
    oracle_lib.build()
    o = ref.options(oracle_lib)
    return dict(alpha=np.full(n, o["relaxLb"]), lb=np.full((1, n), o["lb"]), ub=np.full((1, n), o["ub"]))


def forward(flt, b, T, dt, ld=None):
    """One asif_hip_rollout_params_batch launch with all three logs, in buffers of leading dimension ld."""
    ld = ld or b["x0"].shape[1]
    s = pol._state(b, T, ld)
    flt.rollout_params(T, dt, s["x"], view(b["k"], ld), s["uact"], s["relax"], s["nfail"], K=view(b["K"], ld),
                       v=view(b["v"], ld), alpha=view(b["alpha"], ld), lb=view(b["lb"], ld), ub=view(b["ub"], ld),
                       xlog=s["xlog"], ulog=s["ulog"], rclog=s["rclog"])
    return pol._numpy(s)


def backward(flt, fw, b, T, dt, gxT, guactT=None, gxlog=None, gulog=None, ld=None, gK=True, gv=True, gpar=True):
    """One asif_hip_rollout_params_vjp_batch launch; the WHOLE output buffers (padding included) as numpy; a gradient that
    was not asked for is None."""
    n = b["k"].shape[1]
    ld = ld or n
    sent = lambda *s: padded(np.full(s, SENTINEL), ld)
    out = dict(gx0=sent(2, n), gk=sent(1, n), guact0=sent(1, n), gK=sent(2, n) if gK and b["K"] is not None else None,
               gv=sent(T, 1, n) if gv and b["v"] is not None else None,
               galpha=sent(n) if gpar and b["alpha"] is not None else None,
               glb=sent(1, n) if gpar and b["lb"] is not None else None,
               gub=sent(1, n) if gpar and b["ub"] is not None else None)
    o = lambda k: None if out[k] is None else out[k][1]
    nskip = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    flt.rollout_params_vjp(T, dt, view(fw["xlog"], ld), view(fw["ulog"], ld), view(fw["rclog"], ld, torch.int32),
                           view(b["k"], ld), view(gxT, ld), o("gx0"), o("gk"), o("guact0"), nskip, K=view(b["K"], ld),
                           v=view(b["v"], ld), alpha=view(b["alpha"], ld), lb=view(b["lb"], ld), ub=view(b["ub"], ld),
                           guactT=view(guactT, ld), gxlog=view(gxlog, ld), gulog=view(gulog, ld), gK=o("gK"), gv=o("gv"),
                           galpha=o("galpha"), glb=o("glb"), gub=o("gub"))
    torch.cuda.synchronize()
    res = {k: None if t is None else t[0].cpu().numpy() for k, t in out.items()}
    res["nskip"] = nskip.cpu().numpy()
    return res


def reference(fw, b, dt, keep, gxT, guactT=None, gxlog=None, gulog=None):
    oracle_lib.build()
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], b["k"], b["K"], b["v"], dt, ref.options(oracle_lib, keep), gxT,
                       guactT, gxlog, gulog, b["alpha"], b["lb"], b["ub"])


def check_parity(got, adj, n, what):
    assert np.all(got["nskip"][:n] == 0), f"{what}: nskip != 0 on {(got['nskip'][:n] != 0).sum()} instances"
    scale = (1.0 + adj["S"]) * np.maximum(1.0, 1.0 / adj["amin"])
    worst = 0.0
    for k in GRADS:
        if got[k] is None:
            continue
        gap = np.abs(got[k][..., :n] - adj[k]) / scale
        worst = max(worst, float(gap.max()))
        print(f"{what} {k}: max scaled gap {gap.max():.3e} (bound 1e-9)")
        assert gap.max() <= 1e-9, (what, k, float(gap.max()))
    return worst


SHAPES = [(8, 1e-2, NB, NB), (40, 1e-3, NB, NB), (1, 1e-3, 1, 1), (8, 1e-2, 65, 192)]


@pytest.mark.parametrize("T,dt,n,ld", SHAPES)
def test_without_parameters_both_entries_are_the_policy_entries(hip, T, dt, n, ld):
    """alpha = lb = ub = NULL, and arrays filled with the handle's own values: every output of both entries equals the
    policy entries' bit for bit; in the second case galpha, glb, gub are the reference's."""
    flt = make_filter(hip)
    g = weights(T, n)
    b = batch(T, n, params=())
    want = pol.forward(flt, b, T, dt, ld)
    wantg = pol.backward(flt, want, b, T, dt, *g, ld=ld)
    for name, bb in (("NULL", b), ("the handle's values", dict(b, **handle_params(n)))):
        got = forward(flt, bb, T, dt, ld)
        for k, a in want.items():
            assert np.array_equal(got[k], a), (name, k)
        gotg = backward(flt, got, bb, T, dt, *g, ld=ld)
        for k, a in wantg.items():
            assert np.array_equal(gotg[k], a), (name, k)
        if bb is not b:
            check_parity(gotg, reference(got, bb, dt, 0, *g), n, f"T={T} B={n} handle's values")
            for k in ("galpha", "glb", "gub"):
                assert np.all(gotg[k][..., n:] == SENTINEL), k
            if n == NB:
                assert all(np.any(gotg[k] != 0) for k in ("galpha", "glb", "gub"))
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2), (40, 1e-3, 65, 192, 2)])
def test_forward_step_by_step_on_the_logged_states(hip, T, dt, n, ld, keep):
    """The reference's filter on xlog[t] with the reference's uDes_t and the instance's parameters gives rclog[t] exactly
    and ulog[t] to 1e-6; x_{t+1} is the unfused Euler step of (x_t, u_t) bit for bit; nfail counts rclog < 0; relax is
    alpha_i wherever a step was solved."""
    flt = make_filter(hip, keep)
    b = batch(T, n)
    fw = forward(flt, b, T, dt, ld)
    oracle_lib.build()
    opt = ref.options(oracle_lib, keep)
    par = ref.lane_params(opt, n, b["alpha"], b["lb"], b["ub"])
    assert np.array_equal(fw["xlog"][0], b["x0"])
    prev = b["uprev"][0]
    for t in range(T):
        xt = fw["xlog"][t]
        s = ref.filter_step(xt, ref.policy(b["k"], b["K"], b["v"][t], xt), opt["keep"], *par)
        assert np.array_equal(fw["rclog"][t], np.where(s["ok"], 1, -1)), f"step {t}"
        want = np.where(s["ok"], s["u"], prev)
        assert np.abs(fw["ulog"][t, 0] - want).max() <= 1e-6, f"step {t}"
        assert np.array_equal(fw["ulog"][t, 0][~s["ok"]], prev[~s["ok"]])
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        assert np.array_equal(nxt, ref.plant_step(xt, fw["ulog"][t, 0], dt)), f"step {t}"
        prev = fw["ulog"][t, 0]
    assert np.array_equal(fw["uactT"][0], fw["ulog"][-1, 0])
    assert np.array_equal(fw["nfail"], (fw["rclog"] < 0).sum(axis=0))
    some = (fw["rclog"] > 0).any(axis=0)
    assert np.array_equal(fw["relax"][0][some], b["alpha"][some])
    if n == NB:
        failed = fw["rclog"] < 0
        assert failed.any() and (failed.any(axis=0) & (~failed).any(axis=0)).any()
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2), (40, 1e-3, 65, 192, 2)])
def test_device_sweep_matches_reference_on_device_logs(hip, T, dt, n, ld, keep):
    """Worst gap measured on the MI355X over these shapes: 9.7e-16 of the bound's scale (T = 40, guact0; galpha 1.4e-17,
    glb 4.5e-16, gub 5.1e-16); DESIGN 4.8f."""
    flt = make_filter(hip, keep)
    b = batch(T, n)
    fw = forward(flt, b, T, dt, ld)
    g = weights(T, n)
    got = backward(flt, fw, b, T, dt, *g, ld=ld)
    adj = reference(fw, b, dt, keep, *g)
    check_parity(got, adj, n, f"T={T} dt={dt} B={n} ld={ld} keep={keep}")
    for k in GRADS:
        assert np.all(got[k][..., n:] == SENTINEL), f"{k}: slots >= B written"
    assert np.all(got["nskip"][n:] == -77)
    if (T, n, keep) == (8, NB, 0):
        assert adj["nrow"] >= 100 and adj["nlb"] >= 100 and adj["nub"] >= 100, (adj["nrow"], adj["nlb"], adj["nub"])
    flt.close()


def test_every_optional_parameter_and_gradient(hip):
    """Each parameter given alone, all gradients or none of the three asked for; T = 0 is the identity with zero parameter
    gradients; a batch equals the prefix of a larger one bitwise."""
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    g = weights(T)
    for only in PARAMS:
        b = batch(T, params=(only,))
        fw = forward(flt, b, T, dt)
        check_parity(backward(flt, fw, b, T, dt, *g), reference(fw, b, dt, 0, *g), NB, f"{only} alone")
    b = batch(T)
    fw = forward(flt, b, T, dt)
    full = backward(flt, fw, b, T, dt, *g)
    got = backward(flt, fw, b, T, dt, *g, gpar=False)
    assert got["galpha"] is None and got["glb"] is None and got["gub"] is None
    for k in ("gx0", "gK", "gk", "gv", "guact0", "nskip"):
        assert np.array_equal(got[k], full[k]), k

    m = 200  # a prefix: not a multiple of the wave, more than one of them
    bm = batch(T, m)
    fwm = forward(flt, bm, T, dt)
    for k, a in fw.items():
        assert np.array_equal(fwm[k], a[..., :m]), k
    gm = weights(T, m)
    gotm = backward(flt, fwm, bm, T, dt, *gm)
    for k in GRADS + ("nskip",):
        assert np.array_equal(gotm[k], full[k][..., :m]), k

    b0 = dict(batch(1), v=None)
    fw0 = dict(xlog=np.zeros((0, 2, NB)), ulog=np.zeros((0, 1, NB)), rclog=np.zeros((0, NB), dtype=np.int32))
    g0 = weights(1)
    got = backward(flt, fw0, b0, 0, dt, g0[0], g0[1])
    assert np.array_equal(got["gx0"], g0[0]) and np.array_equal(got["guact0"], g0[1])
    for k in ("gk", "gK", "galpha", "glb", "gub", "nskip"):
        assert np.all(got[k] == 0), k
    s = pol._state(b0, 0, NB)
    flt.rollout_params(0, dt, s["x"], view(b0["k"], NB), s["uact"], s["relax"], s["nfail"], alpha=view(b0["alpha"], NB))
    torch.cuda.synchronize()
    assert np.array_equal(s["x"].cpu().numpy(), b0["x0"]) and np.array_equal(s["uact"].cpu().numpy(), b0["uprev"])
    flt.close()


def test_bad_parameters_are_data(hip):
    """Instances with lb_i > ub_i, alpha_i = NaN and alpha_i = 0, spread over the first waves: every step of such an
    instance fails (rc -1, counted in nfail), its gradients are finite; every other instance is bitwise what it is
    without them."""
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    b = batch(T)
    g = weights(T)
    clean = forward(flt, b, T, dt)
    cleang = backward(flt, clean, b, T, dt, *g)
    bad = dict(b, alpha=b["alpha"].copy(), lb=b["lb"].copy(), ub=b["ub"].copy())
    swapped, nan, zero = np.array([3, 64, 130, 700]), np.array([5, 63, 131, 1500]), np.array([0, 65, 255, 2047])
    bad["lb"][0, swapped], bad["ub"][0, swapped] = b["ub"][0, swapped], b["lb"][0, swapped]
    bad["alpha"][nan] = np.nan
    bad["alpha"][zero] = 0.0
    hit = np.zeros(NB, dtype=bool)
    hit[np.concatenate([swapped, nan, zero])] = True
    fw = forward(flt, bad, T, dt)
    assert np.all(fw["rclog"][:, hit] == -1) and np.all(fw["nfail"][hit] == T)
    assert np.array_equal(fw["uactT"][0][hit], b["uprev"][0][hit])
    for k, a in clean.items():
        assert np.array_equal(fw[k][..., ~hit], a[..., ~hit]), k
    got = backward(flt, fw, bad, T, dt, *g)
    for k in GRADS:
        assert np.all(np.isfinite(got[k][..., hit])), k
        assert np.array_equal(got[k][..., ~hit], cleang[k][..., ~hit]), k
    for k in ("galpha", "glb", "gub", "gk"):
        assert np.all(got[k][..., hit] == 0), k
    assert np.all(got["nskip"] == 0)
    flt.close()


def _segment_loss(outs, g):
    xT, uactT, xlog, ulog = outs[:4]
    return (xT * g[0]).sum() + (uactT * g[1]).sum() + (xlog * g[2]).sum() + (ulog * g[3]).sum()


def test_torch_layer_is_the_two_launches(hip):
    """.backward() gives the direct rollout_params_vjp call's gradients bitwise in one launch; galpha / glb / gub are asked
    for only where the tensor requires a gradient; a shared gain through expand gets the sum of the per-instance galpha."""
    from asif_amd.torch_layer import ParamRolloutLayer
    T, dt = 8, 1e-2
    layer = ParamRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=T, dt=dt)
    calls = []
    inner = layer.filter.rollout_params_vjp
    layer.filter.rollout_params_vjp = lambda *a, **k: (calls.append(k), inner(*a, **k))[1]
    b = batch(T)
    gn = weights(T)
    g = tuple(torch.from_numpy(a).to(DEV) for a in gn)
    args = lambda lv: dict(K=lv["K"], v=lv["v"], uact_prev=lv["uprev"], alpha=lv["alpha"], lb=lv["lb"], ub=lv["ub"])

    lv = pol._leaves(b)
    outs = layer(lv["x0"], lv["k"], **args(lv))
    fw = forward(layer.filter, b, T, dt)
    for o, k in zip(outs, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
        assert np.array_equal(o.detach().cpu().numpy(), fw[k]), k
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    assert len(calls) == 1
    want = backward(layer.filter, fw, b, T, dt, *gn)
    for name, leaf in (("gx0", "x0"), ("gk", "k"), ("gK", "K"), ("gv", "v"), ("guact0", "uprev"), ("galpha", "alpha"),
                       ("glb", "lb"), ("gub", "ub")):
        assert np.array_equal(lv[leaf].grad.cpu().numpy(), want[name]), name

    # only alpha requires a gradient: glb and gub are not asked for
    del calls[:]
    lv = pol._leaves(b)
    outs = layer(lv["x0"].detach(), lv["k"].detach(), **{k: (t if k == "alpha" else t.detach()) for k, t in args(lv).items()})
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0]["galpha"] is not None and calls[0]["glb"] is None and calls[0]["gub"] is None
    assert np.array_equal(lv["alpha"].grad.cpu().numpy(), want["galpha"]) and lv["lb"].grad is None

    # a gain shared by the batch
    shared = torch.tensor([6.0], dtype=torch.float64, device=DEV, requires_grad=True)
    lv = pol._leaves(b)
    outs = layer(lv["x0"], lv["k"], **dict(args(lv), alpha=shared.expand(NB)))
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    bs = dict(b, alpha=np.full(NB, 6.0))
    per = backward(layer.filter, forward(layer.filter, bs, T, dt), bs, T, dt, *gn)["galpha"]
    assert per.sum() != 0 and abs(float(shared.grad[0]) - per.sum()) <= 1e-12 * np.abs(per).sum(), (shared.grad, per.sum())


def test_descent_on_the_barrier_gain_lowers_the_intervention_loss(hip):
    """INTEGRATION.md's example: ten steps of fixed length down the gradient of one shared alpha, from 1.0, lower
    sum |ulog - udes_t|^2.  The states are the workload's scaled into the safe set (x0 / 2), where no step fails: the
    loss is then continuous in alpha (12174 -> 11909 measured, alpha 1.0 -> 2.0).  On the whole workload, a fifth of whose states start
    outside the set, a larger gain makes more steps infeasible, a failed step keeps u_{t-1}, and the loss jumps up at
    each such alpha although its gradient, right wherever it exists, points down."""
    from asif_amd.torch_layer import ParamRolloutLayer
    T, dt = 8, 1e-2
    layer = ParamRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=T, dt=dt)
    b = batch(T, params=())
    t = lambda a: torch.from_numpy(a).to(DEV)
    x0, k, K, v = t(0.5 * b["x0"]), t(b["k"]), t(b["K"]), t(b["v"])
    alpha = torch.tensor([1.0], dtype=torch.float64, device=DEV, requires_grad=True)
    losses = []
    for _ in range(10):
        xT, uactT, xlog, ulog, rclog, nfail = layer(x0, k, K=K, v=v, alpha=alpha.expand(NB))
        udes = k + (K.unsqueeze(0) * xlog).sum(dim=1, keepdim=True) + v
        loss = ((ulog - udes) ** 2).sum()
        grad, = torch.autograd.grad(loss, alpha)
        with torch.no_grad():
            alpha -= 0.1 * grad / grad.abs()  # a step of fixed length down the gradient
        losses.append(float(loss.detach()))
    print("intervention loss per iteration:", [round(x, 3) for x in losses], "alpha ->", float(alpha))
    assert losses[-1] < losses[0]


def test_contract_and_refusals_leave_everything_as_it_was(hip):
    lib = hip.load()
    n, T = 8, 2
    T0, dt0 = 8, 1e-2
    b0, g0 = pol.batch(T0), weights(T0)
    bc = pol.batch(T0, hasK=False, hasV=False)

    def existing():
        """All four existing rollout entries on a fresh handle."""
        flt = make_filter(hip)
        fc = pol.forward_constant(flt, bc, T0, dt0)
        out = [torch.empty((r, NB), dtype=torch.float64, device=DEV) for r in (2, 1, 1)]
        nskip = torch.empty(NB, dtype=torch.int32, device=DEV)
        flt.rollout_vjp(T0, dt0, view(fc["xlog"], NB), view(fc["ulog"], NB), view(fc["rclog"], NB, torch.int32),
                        view(bc["k"], NB), view(g0[0], NB), *out, nskip, guactT=view(g0[1], NB), gxlog=view(g0[2], NB),
                        gulog=view(g0[3], NB))
        torch.cuda.synchronize()
        fp = pol.forward(flt, b0, T0, dt0)
        gp = pol.backward(flt, fp, b0, T0, dt0, *g0)
        flt.close()
        return (list(fc.values()) + [t.cpu().numpy() for t in out] + [nskip.cpu().numpy()] + list(fp.values())
                + list(gp.values()))
    before = existing()

    buf = [torch.ones((T * 2, n), dtype=torch.float64, device=DEV) for _ in range(26)]
    rclog = torch.ones((T, n), dtype=torch.int32, device=DEV)
    ints = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = [C.c_void_p(t.data_ptr()) for t in buf]
    prc, pin = C.c_void_p(rclog.data_ptr()), C.c_void_p(ints.data_ptr())

    def fwd(flt, nb=n, ld=n, steps=T, **null):
        a = dict(x=p[0], K=p[1], k=p[2], v=p[3], alpha=p[17], lb=p[18], ub=p[19], uact=p[4], relax=p[5], nfail=pin,
                 xlog=p[6], ulog=p[7], rclog=prc)
        a.update(null)
        return lib.asif_hip_rollout_params_batch(flt.handle, nb, ld, steps, 1e-3, *a.values(), None)

    def bwd(flt, nb=n, ld=n, steps=T, **null):
        a = dict(xlog=p[6], ulog=p[7], rclog=prc, K=p[1], k=p[2], v=p[3], alpha=p[17], lb=p[18], ub=p[19], gxT=p[8],
                 guactT=p[9], gxlog=p[10], gulog=p[11], gx0=p[12], gK=p[13], gk=p[14], gv=p[15], galpha=p[20], glb=p[21],
                 gub=p[22], guact0=p[16], nskip=pin)
        a.update(null)
        return lib.asif_hip_rollout_params_vjp_batch(flt.handle, nb, ld, steps, 1e-3, *a.values(), None)

    EINVAL, EUNSUPPORTED = -1, -3
    others = [hip.Filter(*hip.CONFIGS[3][:2]), hip.Filter(*hip.CONFIGS[11][:2]),  # implicit; the two-input model
              hip.RealizableFilter(workloads.load_kernel()), hip.RobustDataFilter(workloads.load_halfplanes()),
              make_filter(hip, polish=1), make_filter(hip, polish=0), make_filter(hip, lanes_per_qp=4)]
    for other in others:
        assert fwd(other) == EUNSUPPORTED and bwd(other) == EUNSUPPORTED
        other.close()
    pre = make_filter(hip, polish=1, presolve=1)  # presolve: the light kernel forwards; the sweep wants polish == 2
    assert fwd(pre) == 0 and bwd(pre) == EUNSUPPORTED
    pre.close()
    pre = make_filter(hip, presolve=1)
    assert fwd(pre) == 0 and bwd(pre) == 0
    torch.cuda.synchronize()
    pre.close()

    flt = make_filter(hip)
    for k in ("x", "k", "uact", "relax", "nfail"):
        assert fwd(flt, **{k: None}) == EINVAL, k
    for k in ("xlog", "ulog", "rclog", "k", "gxT", "gx0", "gk", "guact0", "nskip"):
        assert bwd(flt, **{k: None}) == EINVAL, k
    assert bwd(flt, K=None) == EINVAL and bwd(flt, v=None) == EINVAL  # gK without K, gv without v
    for k in PARAMS:  # a gradient asked for a parameter that was not given
        assert bwd(flt, **{k: None}) == EINVAL, k
        assert bwd(flt, **{k: None, "g" + k: None}) == 0, k
    for call in (fwd, bwd):
        assert call(flt, ld=n - 1) == EINVAL and call(flt, steps=-1) == EINVAL and call(flt, nb=-1) == EINVAL
        assert call(flt, nb=0) == 0 and call(flt) == 0
    assert fwd(flt, K=None, v=None, alpha=None, lb=None, ub=None, xlog=None, ulog=None, rclog=None) == 0
    assert fwd(flt, steps=0) == 0
    assert bwd(flt, guactT=None, gxlog=None, gulog=None, gK=None, gv=None, galpha=None, glb=None, gub=None) == 0
    assert bwd(flt, K=None, gK=None, v=None, gv=None, alpha=None, galpha=None, lb=None, glb=None, ub=None, gub=None) == 0
    assert bwd(flt, steps=0, xlog=None, ulog=None, rclog=None) == 0
    torch.cuda.synchronize()

    # still usable: a forward and a backward pass agree with the reference
    Tn, dtn, m = 4, 1e-2, 64
    b = batch(Tn, m)
    fw = forward(flt, b, Tn, dtn)
    g = weights(Tn, m)
    check_parity(backward(flt, fw, b, Tn, dtn, *g), reference(fw, b, dtn, 0, *g), m, "after the refusals")
    flt.close()

    # and all four existing rollout entries, on a fresh handle, give what they gave before any call of the new ones
    for a, c in zip(before, existing()):
        assert (a is None and c is None) or np.array_equal(a, c)
