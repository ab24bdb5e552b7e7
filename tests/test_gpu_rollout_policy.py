"""asif_hip_rollout_policy_batch / asif_hip_rollout_policy_vjp_batch (asif_amd/csrc/k_rollout_policy.hip) and the torch
layer on top of them: the fused explicit rollout under the affine policy uDes_t = k + K x_t + v_t.

Forward: with the policy switched off, asif_hip_rollout_batch bit for bit; with it on, every step checked on the logged
states against the numpy reference of tests/rollout_policy_ref.py (a free-running comparison is meaningless where the
filter's gain blows up, tests/test_gpu_rollout.py).  Backward: the numpy sweep of that file (itself checked against finite
differences in tests/test_rollout_policy_ref_host.py) run on the DEVICE's own logs.

Parity bound per gradient entry: 1e-9 (1 + S_i) max(1, 1 / a_min,i) -- the project's VJP bound with S_i, the largest
magnitude among lambda, mu, d_t and d_t x_t' met along the instance's sweep, in place of |ref| and a_min,i, the smallest
|Lgh| of a safety row active at a solved step, as sigma_min.  No instance is left out.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib
import rollout_policy_ref as ref
from asif_amd import workloads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NB = 2048
SENTINEL = -3.25
GRADS = ("gx0", "gK", "gk", "gv", "guact0")


def make_filter(hip, keep=0, **solver):
    od = hip.default_options(hip.MODEL_DOUBLE_INTEGRATOR, hip.EXPLICIT)
    od.npSSmax = keep
    return hip.Filter(hip.MODEL_DOUBLE_INTEGRATOR, hip.EXPLICIT, options=od,
                      solver=hip.default_solver(**solver) if solver else None)


def batch(T, n=NB, hasK=True, hasV=True):
    """x0, k, K, v, uact_prev: the workload's batch, per-instance gains K ~ (-2, -3) + 0.5 N(0,1), v ~ 0.3 N(0,1)."""
    x0, k = workloads.make_batch(2, NB)
    rng = np.random.default_rng(100)
    uprev = rng.uniform(-1, 1, (1, NB))
    K = np.array([[-2.0], [-3.0]]) + 0.5 * rng.normal(0, 1, (2, NB))
    v = 0.3 * rng.normal(0, 1, (T, 1, NB))
    cut = lambda a: a[..., :n].copy()
    return dict(x0=cut(x0), k=cut(k), K=cut(K) if hasK else None, v=cut(v) if hasV else None, uprev=cut(uprev))


def weights(T, n=NB, seed=0):
    """Fixed random loss weights: gxT, guactT, gxlog, gulog."""
    rng = np.random.default_rng(200 + seed)
    full = (rng.normal(0, 1, (2, NB)), rng.normal(0, 1, (1, NB)), rng.normal(0, 1, (T, 2, NB)), rng.normal(0, 1, (T, 1, NB)))
    return tuple(a[..., :n].copy() for a in full)


def padded(a, ld, dtype=torch.float64, fill=SENTINEL):
    """A device buffer [..., ld] pre-filled with the sentinel holding a in its first columns; returns (buffer, view)."""
    n = a.shape[-1]
    t = torch.full((*a.shape[:-1], ld), fill, dtype=dtype, device=DEV)
    t[..., :n] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t, t[..., :n]


def view(a, ld, dtype=torch.float64):
    return None if a is None else padded(a, ld, dtype, SENTINEL if dtype == torch.float64 else 0)[1]


def _state(b, T, ld):
    n = b["x0"].shape[1]
    s = dict(x=view(b["x0"], ld), uact=view(b["uprev"], ld), relax=view(np.zeros((1, n)), ld),
             nfail=torch.zeros(n, dtype=torch.int32, device=DEV), xlog=view(np.zeros((T, 2, n)), ld),
             ulog=view(np.zeros((T, 1, n)), ld), rclog=view(np.zeros((T, n), dtype=np.int32), ld, torch.int32))
    return s


def _numpy(s):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().copy()
    return dict(xT=g(s["x"]), uactT=g(s["uact"]), relax=g(s["relax"]), xlog=g(s["xlog"]), ulog=g(s["ulog"]),
                rclog=g(s["rclog"]), nfail=g(s["nfail"]))


def forward(flt, b, T, dt, ld=None):
    """One asif_hip_rollout_policy_batch launch with all three logs, in buffers of leading dimension ld."""
    ld = ld or b["x0"].shape[1]
    s = _state(b, T, ld)
    flt.rollout_policy(T, dt, s["x"], view(b["k"], ld), s["uact"], s["relax"], s["nfail"], K=view(b["K"], ld),
                       v=view(b["v"], ld), xlog=s["xlog"], ulog=s["ulog"], rclog=s["rclog"])
    return _numpy(s)


def forward_constant(flt, b, T, dt, ld=None):
    """asif_hip_rollout_batch with udes = k on the same inputs."""
    ld = ld or b["x0"].shape[1]
    s = _state(b, T, ld)
    flt.rollout(T, dt, s["x"], view(b["k"], ld), s["uact"], s["relax"], s["nfail"], s["xlog"], s["ulog"], s["rclog"])
    return _numpy(s)


def backward(flt, fw, b, T, dt, gxT, guactT=None, gxlog=None, gulog=None, ld=None, gK=True, gv=True):
    """One asif_hip_rollout_policy_vjp_batch launch; returns the WHOLE output buffers (padding included) as numpy; a
    gradient that was not asked for is None."""
    n = b["k"].shape[1]
    ld = ld or n
    out = dict(gx0=padded(np.full((2, n), SENTINEL), ld), gk=padded(np.full((1, n), SENTINEL), ld),
               guact0=padded(np.full((1, n), SENTINEL), ld),
               gK=padded(np.full((2, n), SENTINEL), ld) if gK and b["K"] is not None else None,
               gv=padded(np.full((T, 1, n), SENTINEL), ld) if gv and b["v"] is not None else None)
    o = lambda k: None if out[k] is None else out[k][1]
    nskip = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    flt.rollout_policy_vjp(T, dt, view(fw["xlog"], ld), view(fw["ulog"], ld), view(fw["rclog"], ld, torch.int32),
                           view(b["k"], ld), view(gxT, ld), o("gx0"), o("gk"), o("guact0"), nskip, K=view(b["K"], ld),
                           v=view(b["v"], ld), guactT=view(guactT, ld), gxlog=view(gxlog, ld), gulog=view(gulog, ld),
                           gK=o("gK"), gv=o("gv"))
    torch.cuda.synchronize()
    res = {k: None if t is None else t[0].cpu().numpy() for k, t in out.items()}
    res["nskip"] = nskip.cpu().numpy()
    return res


def reference(fw, b, dt, keep, gxT, guactT=None, gxlog=None, gulog=None):
    oracle_lib.build()
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], b["k"], b["K"], b["v"], dt, ref.options(oracle_lib, keep), gxT,
                       guactT, gxlog, gulog)


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
def test_forward_without_a_policy_is_the_rollout_entry(hip, T, dt, n, ld):
    """K = v = NULL, and K, v all zeros: x, uact, relax, nfail, xlog, ulog, rclog of asif_hip_rollout_batch with
    udes = k, bitwise."""
    flt = make_filter(hip)
    b = batch(T, n, hasK=False, hasV=False)
    want = forward_constant(flt, b, T, dt, ld)
    if n == NB:
        failed = want["rclog"] < 0
        assert failed.any() and (~failed).any()
    zeros = dict(b, K=np.zeros((2, n)), v=np.zeros((T, 1, n)))
    for name, bb in (("NULL", b), ("zeros", zeros)):
        got = forward(flt, bb, T, dt, ld)
        for k, a in want.items():
            assert np.array_equal(got[k], a), (name, k)
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2), (40, 1e-3, 65, 192, 2)])
def test_forward_with_the_policy_step_by_step_on_the_logged_states(hip, T, dt, n, ld, keep):
    """The reference's filter on xlog[t] with the reference's uDes_t gives rclog[t] exactly and ulog[t] to 1e-6 (the
    tolerance of tests/test_gpu_rollout.py); x_{t+1} is the unfused Euler step of (x_t, u_t) bit for bit; nfail counts
    rclog < 0."""
    flt = make_filter(hip, keep)
    b = batch(T, n)
    fw = forward(flt, b, T, dt, ld)
    oracle_lib.build()
    opt = ref.options(oracle_lib, keep)
    assert np.array_equal(fw["xlog"][0], b["x0"])
    prev = b["uprev"][0]
    for t in range(T):
        xt = fw["xlog"][t]
        s = ref.filter_step(xt, ref.policy(b["k"], b["K"], b["v"][t], xt), opt)
        assert np.array_equal(fw["rclog"][t], np.where(s["ok"], 1, -1)), f"step {t}"
        want = np.where(s["ok"], s["u"], prev)
        assert np.abs(fw["ulog"][t, 0] - want).max() <= 1e-6, f"step {t}"
        assert np.array_equal(fw["ulog"][t, 0][~s["ok"]], prev[~s["ok"]])
        nxt = fw["xlog"][t + 1] if t + 1 < T else fw["xT"]
        assert np.array_equal(nxt, ref.plant_step(xt, fw["ulog"][t, 0], dt)), f"step {t}"
        prev = fw["ulog"][t, 0]
    assert np.array_equal(fw["uactT"][0], fw["ulog"][-1, 0])
    assert np.array_equal(fw["nfail"], (fw["rclog"] < 0).sum(axis=0))
    if n == NB:
        failed = fw["rclog"] < 0
        assert failed.any() and (failed.any(axis=0) & (~failed).any(axis=0)).any()
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld,keep", [s + (0,) for s in SHAPES] + [(8, 1e-2, NB, NB, 2), (40, 1e-3, 65, 192, 2)])
def test_device_sweep_matches_reference_on_device_logs(hip, T, dt, n, ld, keep):
    """Worst gap measured on the MI355X over these shapes: 9.7e-16 of the bound's scale (T = 40, guact0); DESIGN 4.8e."""
    flt = make_filter(hip, keep)
    b = batch(T, n)
    fw = forward(flt, b, T, dt, ld)
    g = weights(T, n)
    got = backward(flt, fw, b, T, dt, *g, ld=ld)
    check_parity(got, reference(fw, b, dt, keep, *g), n, f"T={T} dt={dt} B={n} ld={ld} keep={keep}")
    for k in GRADS:
        assert np.all(got[k][..., n:] == SENTINEL), f"{k}: slots >= B written"
    assert np.all(got["nskip"][n:] == -77)
    flt.close()


def test_every_optional_input_and_output(hip):
    """Each of K and v present or not (each on its own forward pass); gK / gv asked for or not; each of guactT, gxlog,
    gulog given or not."""
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    gxT, guactT, gxlog, gulog = weights(T)
    for hasK in (True, False):
        for hasV in (True, False):
            b = batch(T, hasK=hasK, hasV=hasV)
            fw = forward(flt, b, T, dt)
            what = f"K given={hasK} v given={hasV}"
            check_parity(backward(flt, fw, b, T, dt, gxT, guactT, gxlog, gulog),
                         reference(fw, b, dt, 0, gxT, guactT, gxlog, gulog), NB, what + ", everything")
            got = backward(flt, fw, b, T, dt, gxT, gK=False, gv=False)
            assert got["gK"] is None and got["gv"] is None
            check_parity(got, reference(fw, b, dt, 0, gxT), NB, what + ", nothing optional")
    b = batch(T)
    fw = forward(flt, b, T, dt)
    for drop in range(3):  # one optional input gradient absent at a time
        opt = [None if j == drop else a for j, a in enumerate((guactT, gxlog, gulog))]
        check_parity(backward(flt, fw, b, T, dt, gxT, *opt), reference(fw, b, dt, 0, gxT, *opt), NB,
                     f"without {('guactT', 'gxlog', 'gulog')[drop]}")
    for gK, gv in ((True, False), (False, True)):
        got = backward(flt, fw, b, T, dt, gxT, guactT, gxlog, gulog, gK=gK, gv=gv)
        assert (got["gK"] is not None) == gK and (got["gv"] is not None) == gv
        check_parity(got, reference(fw, b, dt, 0, gxT, guactT, gxlog, gulog), NB, f"gK asked={gK} gv asked={gv}")
    flt.close()


@pytest.mark.parametrize("T,dt,n,ld", SHAPES)
def test_backward_without_a_policy_is_the_rollout_vjp_entry(hip, T, dt, n, ld):
    """K = v = NULL: gx0, guact0, nskip and gk equal asif_hip_rollout_vjp_batch's gx0, guact0, nskip and gudes, bitwise."""
    flt = make_filter(hip)
    b = batch(T, n, hasK=False, hasV=False)
    fw = forward_constant(flt, b, T, dt, ld)
    g = weights(T, n)
    got = backward(flt, fw, b, T, dt, *g, ld=ld)
    want = {k: padded(np.full((r, n), SENTINEL), ld) for k, r in (("gx0", 2), ("gudes", 1), ("guact0", 1))}
    nskip = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    flt.rollout_vjp(T, dt, view(fw["xlog"], ld), view(fw["ulog"], ld), view(fw["rclog"], ld, torch.int32), view(b["k"], ld),
                    view(g[0], ld), want["gx0"][1], want["gudes"][1], want["guact0"][1], nskip, guactT=view(g[1], ld),
                    gxlog=view(g[2], ld), gulog=view(g[3], ld))
    torch.cuda.synchronize()
    for mine, theirs in (("gx0", "gx0"), ("gk", "gudes"), ("guact0", "guact0")):
        assert np.array_equal(got[mine], want[theirs][0].cpu().numpy()), mine
    assert np.array_equal(got["nskip"], nskip.cpu().numpy())
    if n == NB:
        assert np.abs(got["gk"][:, :n]).max() > 0
    flt.close()


def _segment_loss(outs, g):
    xT, uactT, xlog, ulog = outs[:4]
    return (xT * g[0]).sum() + (uactT * g[1]).sum() + (xlog * g[2]).sum() + (ulog * g[3]).sum()


def _leaves(b):
    return {k: None if a is None else torch.from_numpy(a.copy()).to(DEV).requires_grad_() for k, a in b.items()}


def _direct(flt, outs, lv, T, dt, gxT, guactT=None, gxlog=None, gulog=None):
    """One rollout_policy_vjp call on a layer's own logs, everything asked for; torch tensors."""
    d = lambda t: None if t is None else t.detach().contiguous()
    k = d(lv["k"])
    B = k.shape[1]
    res = dict(gx0=torch.empty((2, B), dtype=torch.float64, device=DEV), gk=torch.empty_like(k), guact0=torch.empty_like(k),
               gK=None if lv["K"] is None else torch.empty((2, B), dtype=torch.float64, device=DEV),
               gv=None if lv["v"] is None else torch.empty((T, 1, B), dtype=torch.float64, device=DEV))
    nskip = torch.empty(B, dtype=torch.int32, device=DEV)
    flt.rollout_policy_vjp(T, dt, d(outs[2]), d(outs[3]), outs[4], k, gxT, res["gx0"], res["gk"], res["guact0"], nskip,
                           K=d(lv["K"]), v=d(lv["v"]), guactT=guactT, gxlog=gxlog, gulog=gulog, gK=res["gK"], gv=res["gv"])
    torch.cuda.synchronize()
    return res


def test_torch_layer_is_the_two_launches(hip):
    """.backward() gives the direct rollout_policy_vjp call's gradients bitwise; one backward launch; an output nobody
    used contributes nothing; rclog / nfail are not differentiable; nothing is launched when nothing asks."""
    from asif_amd.torch_layer import PolicyRolloutLayer
    T, dt = 8, 1e-2
    layer = PolicyRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=T, dt=dt)
    calls = []
    inner = layer.filter.rollout_policy_vjp
    layer.filter.rollout_policy_vjp = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    b = batch(T)
    g = tuple(torch.from_numpy(a).to(DEV) for a in weights(T))

    lv = _leaves(b)
    outs = layer(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"])
    assert not outs[4].requires_grad and not outs[5].requires_grad
    fw = forward(layer.filter, b, T, dt)
    for o, k in zip(outs, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
        assert np.array_equal(o.detach().cpu().numpy(), fw[k]), k
    _segment_loss(outs, g).backward()
    torch.cuda.synchronize()
    assert len(calls) == 1  # (the direct calls below go through the counter too)
    want = _direct(layer.filter, outs, lv, T, dt, *g)
    for name, leaf in (("gx0", "x0"), ("gk", "k"), ("gK", "K"), ("gv", "v"), ("guact0", "uprev")):
        assert torch.equal(lv[leaf].grad, want[name]), name

    # an output nobody used: its gradient arrives as None, and only what is needed is asked for
    del calls[:]
    lv = _leaves(b)
    outs = layer(lv["x0"].detach(), lv["k"], K=lv["K"], v=lv["v"].detach(), uact_prev=lv["uprev"].detach())
    (outs[3] * g[3]).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 1 and lv["x0"].grad is None and lv["v"].grad is None
    want = _direct(layer.filter, outs, lv, T, dt, torch.zeros_like(g[0]), gulog=g[3])
    assert torch.equal(lv["k"].grad, want["gk"]) and torch.equal(lv["K"].grad, want["gK"])

    # nothing requires a gradient: nothing to run backwards
    del calls[:]
    outs = layer(*(torch.from_numpy(b[k]).to(DEV) for k in ("x0", "k")))
    assert not any(t.requires_grad for t in outs) and not calls

    # a gain shared by the batch: autograd's sum over the expanded axis of the per-instance gK
    lv = _leaves(b)
    Ks = torch.tensor([[-2.0], [-3.0]], dtype=torch.float64, device=DEV, requires_grad=True)
    outs = layer(lv["x0"], lv["k"], K=Ks.expand(-1, NB), v=lv["v"], uact_prev=lv["uprev"])
    _segment_loss(outs, g).backward()
    per = _direct(layer.filter, outs, dict(lv, K=Ks.expand(-1, NB)), T, dt, *g)["gK"]
    total = per.sum(dim=1, keepdim=True)
    assert torch.all(total != 0) and torch.all((Ks.grad - total).abs() <= 1e-12 * total.abs()), (Ks.grad, total)

    # T = 0: the identity
    ident = PolicyRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=0, dt=dt)
    lv = _leaves(dict(b, v=np.zeros((0, 1, NB))))
    s = ident(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"])
    assert torch.equal(s[0], lv["x0"]) and torch.equal(s[1], lv["uprev"]) and s[2].shape == (0, 2, NB)
    assert s[4].shape == (0, NB)
    ((s[0] * g[0]).sum() + (s[1] * g[1]).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(lv["x0"].grad, g[0]) and torch.equal(lv["uprev"].grad, g[1])
    assert torch.all(lv["k"].grad == 0.0) and torch.all(lv["K"].grad == 0.0) and lv["v"].grad.shape == (0, 1, NB)


def test_intervention_loss_reaches_the_gains(hip):
    """INTEGRATION.md's example: the loss sum_t (u_t - uDes_t)^2 with uDes_t = k + K xlog[t] + v[t] formed in torch.  K.grad
    is torch's direct part, -2 (u_t - uDes_t) xlog[t]' summed over t, plus the sweep's gK fed gulog = 2 (u_t - uDes_t) and
    gxlog = -2 (u_t - uDes_t) K; against numpy for both parts, within the parity bound with the direct part's magnitude
    (a T-term sum in both: its rounding is far below 1e-9 of it) added to S."""
    from asif_amd.torch_layer import PolicyRolloutLayer
    T, dt = 8, 1e-2
    layer = PolicyRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=T, dt=dt)
    b = batch(T)
    lv = _leaves(b)
    xT, uactT, xlog, ulog, rclog, nfail = layer(lv["x0"], lv["k"], K=lv["K"], v=lv["v"], uact_prev=lv["uprev"])
    udes = lv["k"] + (lv["K"].unsqueeze(0) * xlog).sum(dim=1, keepdim=True) + lv["v"]  # [T,1,B]
    ((ulog - udes) ** 2).sum().backward()
    torch.cuda.synchronize()

    n = lambda t: t.detach().cpu().numpy()
    fw = dict(xlog=n(xlog), ulog=n(ulog), rclog=n(rclog))
    r = fw["ulog"] - (b["k"][None] + (b["K"][None] * fw["xlog"]).sum(axis=1, keepdims=True) + b["v"])  # [T,1,B]
    assert (np.abs(r) > 1e-3).sum() > 1000  # the filter does intervene
    adj = reference(fw, b, dt, 0, np.zeros((2, NB)), None, -2.0 * r * b["K"][None], 2.0 * r)
    direct = (-2.0 * r * fw["xlog"]).sum(axis=0)  # [2,B]
    scale = (1.0 + adj["S"] + np.abs(direct).max(axis=0)) * np.maximum(1.0, 1.0 / adj["amin"])
    gap = np.abs(n(lv["K"].grad) - (direct + adj["gK"])) / scale
    print(f"intervention loss, K.grad: max scaled gap {gap.max():.3e} (bound 1e-9)")
    assert gap.max() <= 1e-9 and np.abs(adj["gK"]).max() > 0


def test_contract_and_refusals_leave_everything_as_it_was(hip):
    lib = hip.load()
    n, T = 8, 2
    # what the existing entries give on a fresh handle before any policy call
    T0, dt0 = 8, 1e-2
    b0, g0 = batch(T0, hasK=False, hasV=False), weights(T0)

    def existing():
        flt = make_filter(hip)
        fw = forward_constant(flt, b0, T0, dt0)
        out = [torch.empty((r, NB), dtype=torch.float64, device=DEV) for r in (2, 1, 1)]
        nskip = torch.empty(NB, dtype=torch.int32, device=DEV)
        flt.rollout_vjp(T0, dt0, view(fw["xlog"], NB), view(fw["ulog"], NB), view(fw["rclog"], NB, torch.int32),
                        view(b0["k"], NB), view(g0[0], NB), *out, nskip, guactT=view(g0[1], NB), gxlog=view(g0[2], NB),
                        gulog=view(g0[3], NB))
        torch.cuda.synchronize()
        flt.close()
        return list(fw.values()) + [t.cpu().numpy() for t in out] + [nskip.cpu().numpy()]
    before = existing()

    buf = [torch.zeros((T * 2, n), dtype=torch.float64, device=DEV) for _ in range(20)]
    rclog = torch.ones((T, n), dtype=torch.int32, device=DEV)
    ints = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = [C.c_void_p(t.data_ptr()) for t in buf]
    prc, pin = C.c_void_p(rclog.data_ptr()), C.c_void_p(ints.data_ptr())

    def fwd(flt, nb=n, ld=n, steps=T, **null):
        a = dict(x=p[0], K=p[1], k=p[2], v=p[3], uact=p[4], relax=p[5], nfail=pin, xlog=p[6], ulog=p[7], rclog=prc)
        a.update(null)
        return lib.asif_hip_rollout_policy_batch(flt.handle, nb, ld, steps, 1e-3, *a.values(), None)

    def bwd(flt, nb=n, ld=n, steps=T, **null):
        a = dict(xlog=p[6], ulog=p[7], rclog=prc, K=p[1], k=p[2], v=p[3], gxT=p[8], guactT=p[9], gxlog=p[10], gulog=p[11],
                 gx0=p[12], gK=p[13], gk=p[14], gv=p[15], guact0=p[16], nskip=pin)
        a.update(null)
        return lib.asif_hip_rollout_policy_vjp_batch(flt.handle, nb, ld, steps, 1e-3, *a.values(), None)

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
    for call in (fwd, bwd):
        assert call(flt, ld=n - 1) == EINVAL and call(flt, steps=-1) == EINVAL and call(flt, nb=-1) == EINVAL
        assert call(flt, nb=0) == 0 and call(flt) == 0
    assert fwd(flt, K=None, v=None, xlog=None, ulog=None, rclog=None) == 0 and fwd(flt, steps=0) == 0
    assert bwd(flt, guactT=None, gxlog=None, gulog=None, gK=None, gv=None) == 0
    assert bwd(flt, K=None, gK=None, v=None, gv=None) == 0
    assert bwd(flt, steps=0, xlog=None, ulog=None, rclog=None) == 0
    torch.cuda.synchronize()

    # still usable: a forward and a backward pass agree with the reference
    Tn, dtn, m = 4, 1e-2, 64
    b = batch(Tn, m)
    fw = forward(flt, b, Tn, dtn)
    g = weights(Tn, m)
    check_parity(backward(flt, fw, b, Tn, dtn, *g), reference(fw, b, dtn, 0, *g), m, "after the refusals")
    flt.close()

    # and the existing entries, on a fresh handle, give what they gave before any policy call
    for a, c in zip(before, existing()):
        assert np.array_equal(a, c)
