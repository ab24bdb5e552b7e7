"""asif_hip_rollout_vjp_batch (asif_amd/csrc/k_rollout_vjp.hip) and the torch layer on top of it, against the numpy sweep
of tests/rollout_vjp_ref.py (itself checked against finite differences in tests/test_rollout_vjp_ref_host.py) run on the
DEVICE's own logs: a free-running comparison is meaningless where the filter's gain blows up (tests/test_gpu_rollout.py).

Parity bound per gradient entry: 1e-9 (1 + S_i) max(1, 1 / a_min,i) -- the project's VJP bound
1e-9 (1 + |ref|) max(1, 1 / sigma_min) with S_i, the largest |lambda| or |mu| met along the instance's sweep, in place of
|ref| (lambda cancels along the sweep) and a_min,i, the smallest |Lgh| of a safety row active at a solved step, as
sigma_min.  No instance is left out.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import oracle_lib
import rollout_vjp_ref as ref
from asif_amd import workloads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NB = 2048
SENTINEL = -3.25


def make_filter(hip, keep=0, **solver):
    od = hip.default_options(hip.MODEL_DOUBLE_INTEGRATOR, hip.EXPLICIT)
    od.npSSmax = keep
    return hip.Filter(hip.MODEL_DOUBLE_INTEGRATOR, hip.EXPLICIT, options=od,
                      solver=hip.default_solver(**solver) if solver else None)


def batch(n=NB, seed=0):
    x0, udes = workloads.make_batch(2, NB)
    rng = np.random.default_rng(100 + seed)
    return x0[:, :n].copy(), udes[:, :n].copy(), rng.uniform(-1, 1, (1, NB))[:, :n].copy()


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


def forward(flt, x0, udes, uprev, T, dt, ld=None):
    """One asif_hip_rollout_batch launch with all three logs, in buffers of leading dimension ld; numpy results."""
    n = x0.shape[1]
    ld = ld or n
    (_, x), (_, u), (_, ua) = padded(x0, ld), padded(udes, ld), padded(uprev, ld)
    _, relax = padded(np.zeros((1, n)), ld)
    nfail = torch.zeros(n, dtype=torch.int32, device=DEV)
    _, xlog = padded(np.zeros((T, 2, n)), ld)
    _, ulog = padded(np.zeros((T, 1, n)), ld)
    _, rclog = padded(np.zeros((T, n), dtype=np.int32), ld, torch.int32, 0)
    flt.rollout(T, dt, x, u, ua, relax, nfail, xlog, ulog, rclog)
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy().copy()
    return dict(xT=g(x), uactT=g(ua), xlog=g(xlog), ulog=g(ulog), rclog=g(rclog), nfail=g(nfail))


def backward(flt, fw, udes, T, dt, gxT, guactT=None, gxlog=None, gulog=None, ld=None):
    """One asif_hip_rollout_vjp_batch launch; returns the WHOLE output buffers (padding included) as numpy."""
    n = udes.shape[1]
    ld = ld or n
    v = lambda a, dt_=torch.float64: None if a is None else padded(a, ld, dt_, SENTINEL if dt_ == torch.float64 else 0)[1]
    out = dict(gx0=padded(np.full((2, n), SENTINEL), ld), gudes=padded(np.full((1, n), SENTINEL), ld),
               guact0=padded(np.full((1, n), SENTINEL), ld))
    nskip = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    flt.rollout_vjp(T, dt, v(fw["xlog"]), v(fw["ulog"]), v(fw["rclog"], torch.int32), v(udes), v(gxT),
                    out["gx0"][1], out["gudes"][1], out["guact0"][1], nskip, guactT=v(guactT), gxlog=v(gxlog),
                    gulog=v(gulog))
    torch.cuda.synchronize()
    res = {k: t[0].cpu().numpy() for k, t in out.items()}
    res["nskip"] = nskip.cpu().numpy()
    return res


def reference(fw, udes, dt, keep, gxT, guactT=None, gxlog=None, gulog=None):
    oracle_lib.build()
    return ref.adjoint(fw["xlog"], fw["ulog"], fw["rclog"], udes, dt, ref.options(oracle_lib, keep), gxT, guactT, gxlog,
                       gulog)


def check_parity(got, adj, n, what):
    assert np.all(got["nskip"][:n] == 0), f"{what}: nskip != 0 on {(got['nskip'][:n] != 0).sum()} instances"
    scale = (1.0 + adj["S"]) * np.maximum(1.0, 1.0 / adj["amin"])
    worst = 0.0
    for k in ("gx0", "gudes", "guact0"):
        gap = np.abs(got[k][:, :n] - adj[k]) / scale[None, :]
        worst = max(worst, float(gap.max()))
        print(f"{what} {k}: max scaled gap {gap.max():.3e} (bound 1e-9)")
        assert gap.max() <= 1e-9, (what, k, float(gap.max()), int(gap.max(axis=0).argmax()))
    return worst


@pytest.mark.parametrize("T,dt,n,ld,keep", [(8, 1e-2, NB, NB, 0), (40, 1e-3, NB, NB, 0), (1, 1e-3, 1, 1, 0),
                                            (8, 1e-2, 65, 192, 0), (8, 1e-2, NB, NB, 2), (40, 1e-3, 65, 192, 2)])
def test_device_sweep_matches_reference_on_device_logs(hip, T, dt, n, ld, keep):
    """Worst gap measured on the MI355X over these shapes: 9.7e-16 of the bound's scale (T = 40, guact0); DESIGN 4.8d."""
    flt = make_filter(hip, keep)
    x0, udes, uprev = batch(n)
    fw = forward(flt, x0, udes, uprev, T, dt, ld)
    if n == NB:  # the batch has failed steps and instances that fail and recover
        failed = fw["rclog"] < 0
        assert failed.any() and (failed.any(axis=0) & (~failed).any(axis=0)).any()
    g = weights(T, n)
    got = backward(flt, fw, udes, T, dt, *g, ld=ld)
    check_parity(got, reference(fw, udes, dt, keep, *g), n, f"T={T} dt={dt} B={n} ld={ld} keep={keep}")
    for k in ("gx0", "gudes", "guact0"):
        assert np.all(got[k][:, n:] == SENTINEL), f"{k}: slots >= B written"
    assert np.all(got["nskip"][n:] == -77)
    flt.close()


def test_every_combination_of_optional_inputs(hip):
    T, dt = 8, 1e-2
    flt = make_filter(hip)
    x0, udes, uprev = batch()
    fw = forward(flt, x0, udes, uprev, T, dt)
    gxT, guactT, gxlog, gulog = weights(T)
    for use in itertools.product((False, True), repeat=3):
        opt = [a if u else None for a, u in zip((guactT, gxlog, gulog), use)]
        got = backward(flt, fw, udes, T, dt, gxT, *opt)
        check_parity(got, reference(fw, udes, dt, 0, gxT, *opt), NB, f"guactT/gxlog/gulog given={use}")
    flt.close()


def test_one_step_ties_to_the_filter_vjp_kernel(hip):
    """T = 1 without log gradients: gudes is what asif_hip_filter_vjp_batch gives for guact = guactT + dt g' gxT on
    solved instances, to 1e-15 (1 + |ref|); a failed instance hands exactly that guact on as guact0."""
    dt = 1e-2
    flt = make_filter(hip)
    x0, udes, uprev = batch()
    fw = forward(flt, x0, udes, uprev, 1, dt)
    gxT, guactT, _, _ = weights(1)
    got = backward(flt, fw, udes, 1, dt, gxT, guactT)
    guact = guactT + dt * (0.0 * gxT[0] + 1.0 * gxT[1])[None, :]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    gudes = torch.zeros((1, NB), dtype=torch.float64, device=DEV)
    rc = torch.zeros(NB, dtype=torch.int32, device=DEV)
    flt.filter_vjp(t(x0), t(udes), t(guact), gudes, rc)
    torch.cuda.synchronize()
    rc, gudes = rc.cpu().numpy(), gudes.cpu().numpy()
    assert np.array_equal(rc, fw["rclog"][0])
    ok = rc == 1
    assert ok.sum() > 1000 and (~ok).sum() > 400
    gap = np.abs(got["gudes"] - gudes) / (1.0 + np.abs(gudes))
    assert gap[:, ok].max() <= 1e-15, float(gap[:, ok].max())
    assert np.array_equal(got["guact0"][:, ~ok], guact[:, ~ok])
    assert np.all(got["guact0"][:, ok] == 0.0) and np.all(got["gudes"][:, ~ok] == 0.0)
    flt.close()


def test_a_batch_equals_the_prefix_of_a_larger_one(hip):
    T, dt, n = 8, 1e-2, 100
    flt = make_filter(hip)
    x0, udes, uprev = batch()
    g = weights(T)
    fw = forward(flt, x0, udes, uprev, T, dt)
    full = backward(flt, fw, udes, T, dt, *g)
    fws = forward(flt, x0[:, :n].copy(), udes[:, :n].copy(), uprev[:, :n].copy(), T, dt)
    for k in ("xT", "uactT", "xlog", "ulog", "rclog"):
        assert np.array_equal(fws[k], fw[k][..., :n]), k
    small = backward(flt, fws, udes[:, :n].copy(), T, dt, *(a[..., :n].copy() for a in g))
    for k in ("gx0", "gudes", "guact0"):
        assert np.array_equal(small[k], full[k][:, :n]), k
    flt.close()


def _segment_loss(outs, g):
    gxT, guactT, gxlog, gulog = g
    xT, uactT, xlog, ulog = outs[:4]
    return (xT * gxT).sum() + (uactT * guactT).sum() + (xlog * gxlog).sum() + (ulog * gulog).sum()


def test_two_chained_segments_are_one_sweep_cut_in_two(hip):
    from asif_amd.torch_layer import ExplicitRolloutFn
    T1, T2, dt = 3, 5, 1e-2
    flt = make_filter(hip)
    x0n, udesn, uprevn = batch()
    g = tuple(torch.from_numpy(a).to(DEV) for a in weights(T1 + T2))
    leaves = lambda: tuple(torch.from_numpy(a.copy()).to(DEV).requires_grad_() for a in (x0n, udesn, uprevn))

    x0, udes, uprev = leaves()
    one = ExplicitRolloutFn.apply(flt, x0, udes, uprev, T1 + T2, dt)
    _segment_loss(one, g).backward()

    y0, vdes, vprev = leaves()
    a = ExplicitRolloutFn.apply(flt, y0, vdes, vprev, T1, dt)
    b = ExplicitRolloutFn.apply(flt, a[0], vdes, a[1], T2, dt)
    two = (b[0], b[1], torch.cat([a[2], b[2]]), torch.cat([a[3], b[3]]), torch.cat([a[4], b[4]]), a[5] + b[5])
    _segment_loss(two, g).backward()
    torch.cuda.synchronize()

    for p, q, k in zip(one, two, ("xT", "uactT", "xlog", "ulog", "rclog", "nfail")):
        assert torch.equal(p, q), k
    failed = one[4].cpu().numpy() < 0
    assert (failed.any(axis=0) & (~failed).any(axis=0)).sum() > 0  # instances that fail and recover
    assert torch.equal(x0.grad, y0.grad) and torch.equal(uprev.grad, vprev.grad)
    fw = dict(xlog=one[2].detach().cpu().numpy(), ulog=one[3].detach().cpu().numpy(), rclog=one[4].cpu().numpy())
    adj = reference(fw, udesn, dt, 0, *(t.cpu().numpy() for t in g))
    gap = np.abs(udes.grad.cpu().numpy() - vdes.grad.cpu().numpy())[0] / (1.0 + adj["S"])
    print(f"gudes, one sweep against two: max gap {gap.max():.3e} of 1 + S (bound 1e-13)")
    assert gap.max() <= 1e-13
    check_parity(dict(gx0=x0.grad.cpu().numpy(), gudes=udes.grad.cpu().numpy(), guact0=uprev.grad.cpu().numpy(),
                      nskip=np.zeros(NB, dtype=np.int32)), adj, NB, "torch, T = 8")
    flt.close()


def test_torch_layer_end_to_end(hip):
    """Two segments with a small linear policy udes = W x + b between them; .backward() gives the reference's gradients:
    each segment's sweep against the numpy sweep on the segment's own logs and incoming gradients, and the policy's
    chain rule on top.  One backward launch per segment; none when nothing asks for a gradient; T = 0 is the identity."""
    from asif_amd.torch_layer import ExplicitRolloutLayer
    T, dt = 4, 1e-2
    layer = ExplicitRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=T, dt=dt)
    calls = []
    inner = layer.filter.rollout_vjp
    layer.filter.rollout_vjp = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    x0n, _, uprevn = batch()
    W = torch.tensor([[-0.7, -1.1]], dtype=torch.float64, device=DEV, requires_grad=True)
    bias = torch.tensor([[0.05]], dtype=torch.float64, device=DEV, requires_grad=True)
    x0 = torch.from_numpy(x0n).to(DEV).requires_grad_()
    g1, g2 = (tuple(torch.from_numpy(a).to(DEV) for a in weights(T, seed=s)) for s in (1, 2))

    u1 = W @ x0 + bias
    s1 = layer(x0, u1, torch.from_numpy(uprevn).to(DEV))
    u2 = W @ s1[0] + bias
    s2 = layer(s1[0], u2, s1[1])
    for t in (u1, u2, s1[0], s1[1]):
        t.retain_grad()
    assert not s1[4].requires_grad and not s1[5].requires_grad
    (_segment_loss(s1, g1) + _segment_loss(s2, g2)).backward()
    torch.cuda.synchronize()
    assert len(calls) == 2

    n = lambda t: t.detach().cpu().numpy()
    Wn = n(W)
    logs = lambda s: dict(xlog=n(s[2]), ulog=n(s[3]), rclog=n(s[4]))
    # segment 2: the loss's own weights come in
    adj2 = reference(logs(s2), n(u2), dt, 0, *(n(t) for t in g2))
    check_parity(dict(gx0=n(s1[0].grad) - Wn.T @ n(u2.grad) - n(g1[0]), gudes=n(u2.grad),
                      guact0=n(s1[1].grad) - n(g1[1]), nskip=np.zeros(NB, dtype=np.int32)), adj2, NB, "segment 2")
    # segment 1: what came down from segment 2 plus the loss's own weights
    adj1 = reference(logs(s1), n(u1), dt, 0, n(s1[0].grad), n(s1[1].grad), n(g1[2]), n(g1[3]))
    got_gx0 = n(x0.grad) - Wn.T @ n(u1.grad)
    check_parity(dict(gx0=got_gx0, gudes=n(u1.grad), guact0=adj1["guact0"], nskip=np.zeros(NB, dtype=np.int32)), adj1, NB,
                 "segment 1")
    # the policy's parameters: torch's own chain rule on the two gudes
    gW = n(u1.grad) @ x0n.T + n(u2.grad) @ n(s1[0]).T
    np.testing.assert_allclose(n(W.grad), gW, rtol=1e-12, atol=1e-12 * np.abs(gW).max())
    np.testing.assert_allclose(n(bias.grad), (n(u1.grad) + n(u2.grad)).sum(axis=1, keepdims=True), rtol=1e-12)

    # nothing requires a gradient: nothing to run backwards
    del calls[:]
    s = layer(x0.detach(), u1.detach(), s1[1].detach())
    assert not any(t.requires_grad for t in s) and not calls
    # an output nobody used: its gradient arrives as None
    xd = x0.detach().clone().requires_grad_()
    s = layer(xd, u1.detach())
    (s[3] * g1[3]).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 1
    only = reference(logs(s), n(u1), dt, 0, np.zeros((2, NB)), None, None, n(g1[3]))
    check_parity(dict(gx0=n(xd.grad), gudes=only["gudes"], guact0=only["guact0"], nskip=np.zeros(NB, dtype=np.int32)),
                 only, NB, "gulog only")

    # T = 0: the identity
    ident = ExplicitRolloutLayer(hip.MODEL_DOUBLE_INTEGRATOR, T=0, dt=dt)
    xi = x0.detach().clone().requires_grad_()
    ui = u1.detach().clone().requires_grad_()
    pi = torch.from_numpy(uprevn).to(DEV).requires_grad_()
    s = ident(xi, ui, pi)
    assert torch.equal(s[0], xi) and torch.equal(s[1], pi) and s[2].shape == (0, 2, NB) and s[4].shape == (0, NB)
    ((s[0] * g1[0]).sum() + (s[1] * g1[1]).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(xi.grad, g1[0]) and torch.equal(pi.grad, g1[1]) and torch.all(ui.grad == 0.0)


def test_refusals_leave_the_handle_usable(hip):
    lib = hip.load()
    n, T = 8, 2
    buf = [torch.zeros((T * 2, n), dtype=torch.float64, device=DEV) for _ in range(11)]
    rclog = torch.ones((T, n), dtype=torch.int32, device=DEV)
    nskip = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = [C.c_void_p(b.data_ptr()) for b in buf]
    prc, pns = C.c_void_p(rclog.data_ptr()), C.c_void_p(nskip.data_ptr())

    def call(flt, nb=n, ld=n, steps=T, **null):
        a = dict(xlog=p[0], ulog=p[1], rclog=prc, udes=p[2], gxT=p[3], guactT=p[4], gxlog=p[5], gulog=p[6], gx0=p[7],
                 gudes=p[8], guact0=p[9], nskip=pns)
        a.update(null)
        return lib.asif_hip_rollout_vjp_batch(flt.handle, nb, ld, steps, 1e-3, *a.values(), None)

    EINVAL, EUNSUPPORTED = -1, -3
    for cfg in (3, 11):  # an implicit handle, the two-input model
        other = hip.Filter(*hip.CONFIGS[cfg][:2])
        assert call(other) == EUNSUPPORTED
        other.close()
    pol = make_filter(hip, polish=1)
    assert call(pol) == EUNSUPPORTED
    pol.close()
    flt = make_filter(hip)
    for k in ("xlog", "ulog", "rclog", "udes", "gxT", "gx0", "gudes", "guact0", "nskip"):
        assert call(flt, **{k: None}) == EINVAL, k
    assert call(flt, ld=n - 1) == EINVAL and call(flt, steps=-1) == EINVAL and call(flt, nb=-1) == EINVAL
    assert call(flt, nb=0) == 0
    assert call(flt, guactT=None, gxlog=None, gulog=None) == 0 and call(flt) == 0
    assert call(flt, steps=0, xlog=None, ulog=None, rclog=None) == 0
    torch.cuda.synchronize()
    pre = make_filter(hip, presolve=1)
    assert call(pre) == 0
    torch.cuda.synchronize()
    pre.close()
    # still usable: a forward and a backward pass agree with the reference
    x0, udes, uprev = batch(64)
    fw = forward(flt, x0, udes, uprev, 4, 1e-2)
    g = weights(4, 64)
    check_parity(backward(flt, fw, udes, 4, 1e-2, *g), reference(fw, udes, 1e-2, 0, *g), 64, "after the refusals")
    flt.close()
