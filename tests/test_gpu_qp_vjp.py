"""asif_hip_qp_vjp_batch (asif_amd/csrc/k_qp_vjp.hip) and QPSolveFn / QPLayer on top of it, against the numpy adjoint of
tests/qp_vjp_ref.py (itself checked against finite differences of the oracle in tests/test_qp_vjp_host.py).

Parity bound per gradient entry: 1e-9 (1 + |ref|) max(1, 1 / sigma_min(N D^-1/2)), the bound of
tests/test_gpu_explicit_vjp.py: a gradient is a rational function of x* and the active rows with conditioning
1 / sigma_min, and a wrong working set is an O(1) error.  Instances the reference flags degenerate are left out: at most
1 % of a case, asserted.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import oracle_lib
import qp_vjp_ref as ref
import vjp_ref
from asif_amd import workloads

pytestmark = pytest.mark.gpu

B = 1000  # no multiple of 256, nor of 64 / G
DEV = "cuda:0"
OUTS = (*ref.GRADS, "sol")
# both sides of every switch between instantiations: <NV, 8, 1> up to 8 rows, <NV, 48, 4> from 9 on
SHAPES = [(2, 1), (2, 4), (2, 8), (2, 9), (2, 18), (2, 48), (3, 1), (3, 8), (3, 9), (3, 17), (3, 41), (3, 48)]


@functools.lru_cache(maxsize=None)
def case(nv, nc, kind):
    """One batch and its reference; computed once, shared, never written to."""
    oracle_lib.build()
    q = ref.family(nv, nc, kind, B)
    r = ref.adjoint(oracle_lib, q)
    for a in (*q.values(), *r.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return q, r


def rows_of(q, k):
    nv, nc = q["nv"], q["nc"]
    return {"gA": nv * nc, "A": nv * nc, "gb": nc, "b": nc}.get(k, nv)


def run_vjp(hip, q, n=None, ld=None, sentinel=0.0, outs=OUTS):
    """One qp_vjp_batch call on the first n instances of q (AoS numpy) in SoA buffers of leading dimension ld that
    were filled with `sentinel`; outputs not named in `outs` are passed as NULL.  Returns the whole buffers, AoS."""
    n = q["c"].shape[0] if n is None else n
    ld = ld or max(n, 1)

    def up(a):
        t = torch.full((a.shape[1], ld), sentinel, dtype=torch.float64, device=DEV)
        t[:, :n] = torch.from_numpy(np.array(a[:n].T))
        return t

    ins = {k: up(q[k]) for k in ("Hd", "c", "A", "b", "lb", "ub", "gsol")}
    res = {k: torch.full((rows_of(q, k), ld), sentinel, dtype=torch.float64, device=DEV) for k in outs}
    rc = torch.full((ld,), -77, dtype=torch.int32, device=DEV)
    v = lambda t: t[:, :n]  # shape [rows, n], stride ld
    hip.qp_vjp_batch(*(v(ins[k]) for k in ("Hd", "c", "A", "b", "lb", "ub", "gsol")), rc,
                     **{k: v(t) for k, t in res.items()}, be=q["be"])
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy().T.copy() for k, t in res.items()}
    got["rc"] = rc.cpu().numpy()
    return got


def usable(r):
    ok = r["rc"] == 1
    assert (ok & r["degenerate"]).sum() <= 0.01 * len(ok), "more than 1 % of the case is flagged degenerate"
    return ok & ~r["degenerate"]


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("nv,nc", SHAPES)
def test_parity(hip, nv, nc, kind):
    q, r = case(nv, nc, kind)
    got = run_vjp(hip, q)
    assert np.array_equal(got["rc"], r["rc"]), f"{(got['rc'] != r['rc']).sum()} rc mismatches"
    assert np.all(r["rc"] == 1)
    good = usable(r)
    scale = np.maximum(1.0, 1.0 / r["smin"])[:, None]
    worst = 0.0
    for k in ref.GRADS:
        gap = np.abs(got[k] - r[k]) / ((1.0 + np.abs(r[k])) * scale)
        w = float(gap[good].max())
        worst = max(worst, w)
        assert w <= 1e-9, (k, w, int(np.argmax(gap[good].max(axis=1))))
        if k in ("gA", "gb", "glb", "gub"):  # rows and bounds outside the working set: exactly zero
            assert np.all(got[k][good][r[k][good] == 0.0] == 0.0), k
    dsol = float(np.abs(got["sol"] - r["sol"]).max())
    print(f"gpu {nv}x{nc} {kind}: max scaled gap {worst:.3e}, max |sol - oracle| {dsol:.3e}")
    assert dsol <= 1e-12


@pytest.mark.parametrize("nv,nc", [(2, 4), (3, 9)])
def test_layout(hip, nv, nc):
    """Slots beyond B keep their sentinel; NULL for any subset of the outputs leaves the others bitwise as they are
    with every output given; B = 1 and B = 0 work."""
    q, _ = case(nv, nc, "pinned")
    full = run_vjp(hip, q)
    pad = run_vjp(hip, q, ld=B + 37, sentinel=-3.25)
    for k in OUTS:
        assert np.all(pad[k][B:] == -3.25), f"{k}: slots >= B written"
        assert np.array_equal(pad[k][:B], full[k]), k
    assert np.all(pad["rc"][B:] == -77) and np.array_equal(pad["rc"][:B], full["rc"])
    for m in range(len(OUTS)):
        for outs in itertools.combinations(OUTS, m):
            got = run_vjp(hip, q, outs=outs)
            assert np.array_equal(got["rc"], full["rc"])
            for k in outs:
                assert np.array_equal(got[k], full[k]), (outs, k)
    one = run_vjp(hip, q, n=1, ld=64, sentinel=-3.25)
    for k in OUTS:
        assert np.array_equal(one[k][:1], full[k][:1]) and np.all(one[k][1:] == -3.25), k
    assert one["rc"][0] == full["rc"][0] and np.all(one["rc"][1:] == -77)
    none = run_vjp(hip, q, n=0, ld=64, sentinel=-3.25)
    assert all(np.all(none[k] == -3.25) for k in OUTS) and np.all(none["rc"] == -77)


@pytest.mark.parametrize("nv,nc", [(2, 4), (3, 17)])
def test_mixed_batch(hip, nv, nc):
    """Plain, pinned, infeasible, NaN and Hd = 0 instances interleaved: the solved ones receive, bit for bit, what they
    receive in a batch of solved instances only -- an instance's working set must not depend on its wave neighbours,
    which is why the kernel calls solve_general directly -- and the others rc -1 / -1 / 0 and all-zero gradients."""
    plain, pinned = case(nv, nc, "plain")[0], case(nv, nc, "pinned")[0]
    n = 5 * 200
    how = np.arange(n) % 5
    q = dict(nv=nv, nc=nc, be=plain["be"])
    for k in ("Hd", "c", "A", "b", "lb", "ub", "gsol"):
        q[k] = np.where((how == 1)[:, None], pinned[k][:n], plain[k][:n])
    A = q["A"].reshape(n, nv, nc)
    bad = how == 2  # row 1 = -row 0 with a right side that excludes row 0:  a.x >= b  and  a.x <= b - 1
    A[bad, :, 1] = -A[bad, :, 0]
    q["b"][bad, 1] = -q["b"][bad, 0] + 1.0
    A[how == 3, nv - 1, 1] = np.nan  # row 1: with a lane group, a row that lane 0 of the group does not own
    q["gsol"][how == 3, 0] = np.inf  # nothing of an unsolved instance may leak into its slots
    q["Hd"][how == 4, 0] = 0.0
    want = np.choose(how, [1, 1, -1, -1, 0]).astype(np.int32)
    got = run_vjp(hip, q)
    assert np.array_equal(got["rc"], want)
    for k in ref.GRADS:
        assert np.all(got[k][want != 1] == 0.0), k
    solved = {k: (v[want == 1] if isinstance(v, np.ndarray) and k != "be" else v) for k, v in q.items()}
    alone = run_vjp(hip, solved)
    assert np.all(alone["rc"] == 1)
    for k in OUTS:
        assert np.array_equal(got[k][want == 1], alone[k]), k


def test_agrees_with_the_explicit_filter_vjp(hip):
    """Config 2 (DoubleIntegrator), 4096 states: the rows of Filter.assemble with the cost and bounds the explicit
    class gives its QP (k_explicit_vjp.hip) and gsol = [guact, 0] must give -2 gc[0] = gudes of filter_vjp and the same
    rc.  The two eliminate the pinned relaxation variable differently, so the comparison is within the parity bound."""
    n = 4096
    oracle_lib.build()
    x, udes = workloads.make_batch(2, n)
    guact = np.random.default_rng(2).normal(0, 1, (1, n))
    r = vjp_ref.vjp(oracle_lib, 2, x, udes, guact)
    flt = hip.Filter(*hip.CONFIGS[2][:2])
    d, o = flt.dims, flt.options
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xd, ud, gd = t(x), t(udes), t(guact)
    A = torch.zeros((d.nc * d.nv, n), dtype=torch.float64, device=DEV)
    b = torch.zeros((d.nc, n), dtype=torch.float64, device=DEV)
    code = torch.zeros(n, dtype=torch.int32, device=DEV)
    flt.assemble(xd, A, b, code)
    gudes = torch.zeros((1, n), dtype=torch.float64, device=DEV)
    rc_e = torch.zeros(n, dtype=torch.int32, device=DEV)
    flt.filter_vjp(xd, ud, gd, gudes, rc_e)
    one = torch.ones((1, n), dtype=torch.float64, device=DEV)
    Hd = torch.cat([one, o.relaxCost * one])
    c = torch.cat([-2.0 * ud, -2.0 * o.relaxCost * o.relaxLb * one])
    lb = torch.cat([o.lb[0] * one, o.relaxLb * one])
    ub = torch.cat([o.ub[0] * one, o.relaxLb * one])
    gsol = torch.cat([gd, 0.0 * one])
    gc = torch.zeros((2, n), dtype=torch.float64, device=DEV)
    rc_q = torch.zeros(n, dtype=torch.int32, device=DEV)
    hip.qp_vjp_batch(Hd, c, A, b, lb, ub, gsol, rc_q, gc=gc)
    torch.cuda.synchronize()
    flt.close()
    assert torch.equal(rc_q, rc_e) and np.array_equal(rc_q.cpu().numpy(), r["rc"])
    ok = r["rc"] == 1
    good = ok & ~r["degenerate"]
    assert (ok & r["degenerate"]).sum() <= 0.01 * n and good.sum() > 2000
    want, got = gudes.cpu().numpy()[0], -2.0 * gc.cpu().numpy()[0]
    gap = np.abs(got - want) / ((1.0 + np.abs(want)) * np.maximum(1.0, 1.0 / r["smin"]))
    print(f"explicit VJP against QP VJP: max scaled gap {gap[good].max():.3e}")
    assert gap[good].max() <= 1e-9
    assert (want[good] != 0.0).any() and (want[good] == 0.0).any()  # free and blocked inputs both occur
    assert np.all(got[~ok] == 0.0)


def soa(q, k, n=B):
    return torch.from_numpy(np.ascontiguousarray(q[k][:n].T)).to(DEV)


def test_autograd_function_is_the_direct_call(hip, monkeypatch):
    from asif_amd.torch_layer import QPLayer, QPSolveFn
    q, _ = case(3, 17, "eqrow")
    names = ("Hd", "c", "A", "b", "lb", "ub")
    ins = [soa(q, k).requires_grad_() for k in names]
    gsol = soa(q, "gsol")
    sol, status = QPLayer(q["be"])(*ins)
    assert sol.requires_grad and not status.requires_grad and status.dtype == torch.int32
    (sol * gsol).sum().backward()
    torch.cuda.synchronize()
    direct = run_vjp(hip, q)
    assert np.array_equal(status.cpu().numpy(), direct["rc"])
    for t, k in zip(ins, ref.GRADS):
        assert np.array_equal(t.grad.cpu().numpy().T, direct[k]), k
    fwd = torch.zeros_like(sol)
    st = torch.zeros_like(status)
    hip.qp_solve_batch(*(t.detach() for t in ins), fwd, st, be=q["be"])
    assert torch.equal(fwd, sol.detach()) and torch.equal(st, status)

    # gradients are allocated, and asked of the kernel, only where an input requires them
    seen = []
    real = hip.qp_vjp_batch
    monkeypatch.setattr(hip, "qp_vjp_batch", lambda *a, **kw: (seen.append(kw), real(*a, **kw))[1])
    ins = [soa(q, k) for k in names]
    ins[1].requires_grad_()
    ins[3].requires_grad_()
    sol, _ = QPSolveFn.apply(*ins, q["be"])
    (sol * gsol).sum().backward()
    torch.cuda.synchronize()
    assert len(seen) == 1, "backward is one launch"
    assert {k for k in ref.GRADS if seen[0].get(k) is not None} == {"gc", "gb"}
    assert np.array_equal(ins[1].grad.cpu().numpy().T, direct["gc"]) and ins[0].grad is None
    assert np.array_equal(ins[3].grad.cpu().numpy().T, direct["gb"])


def test_toy_model_trains_through_the_qp(hip):
    """c = -2 mlp(x) in front of a 2 x 4 QP, loss on sol: the gradient reaches the MLP's weights."""
    from asif_amd.torch_layer import QPLayer
    q, _ = case(2, 4, "plain")
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.Tanh(), torch.nn.Linear(16, 2)).double().to(DEV)
    feat = torch.randn(B, 3, dtype=torch.float64, device=DEV)
    c = -2.0 * mlp(feat).T
    sol, status = QPLayer()(soa(q, "Hd"), c, soa(q, "A"), soa(q, "b"), soa(q, "lb"), soa(q, "ub"))
    assert bool((status == 1).all())
    ((sol - 0.25) ** 2).sum().backward()
    for p in mlp.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0


def test_argument_contract(hip):
    from asif_amd.torch_layer import QPSolveFn
    q, _ = case(2, 4, "plain")
    good = [soa(q, k, 8) for k in ("Hd", "c", "A", "b", "lb", "ub")]
    for i, wrong in ((0, good[0].float()), (2, good[2][:-1]), (4, good[4].cpu()), (5, good[5][:, :-1])):
        args = list(good)
        args[i] = wrong
        with pytest.raises(ValueError):
            QPSolveFn.apply(*args, None)
    with pytest.raises(ValueError):
        QPSolveFn.apply(*good, [0, 1])  # four rows, two flags
    with pytest.raises(ValueError):
        QPSolveFn.apply(good[0][:1], good[1][:1], good[2][:4], good[3], good[4][:1], good[5][:1], None)  # nv = 1

    lib = hip.load()
    p = [C.c_void_p(t.data_ptr()) for t in good]
    g = torch.zeros((2, 8), dtype=torch.float64, device=DEV)
    rc = torch.zeros(8, dtype=torch.int32, device=DEV)
    pg, prc = C.c_void_p(g.data_ptr()), C.c_void_p(rc.data_ptr())

    def call(n, ld, nv, nc, ins=p, gsol=pg, rcp=prc):
        return lib.asif_hip_qp_vjp_batch(0, n, ld, nv, nc, *ins, None, gsol, None, None, None, None, None, None, None,
                                         rcp, None)

    EINVAL, EUNSUPPORTED = -1, -3
    assert call(8, 8, 2, 4) == 0
    assert call(0, 8, 2, 4) == 0 and call(0, 0, 3, 48, ins=[None] * 6, gsol=None, rcp=None) == 0
    assert call(8, 7, 2, 4) == EINVAL and call(-1, 8, 2, 4) == EINVAL and call(8, 8, 2, -1) == EINVAL
    assert call(8, 8, 2, 4, gsol=None) == EINVAL and call(8, 8, 2, 4, rcp=None) == EINVAL
    assert call(8, 8, 2, 4, ins=[None] + p[1:]) == EINVAL
    for nv, nc in ((1, 4), (4, 4), (2, 0), (2, 49), (3, 49)):
        assert call(8, 8, nv, nc) == EUNSUPPORTED, (nv, nc)
    torch.cuda.synchronize()


def test_forward_untouched(hip):
    q, _ = case(3, 41, "plain")
    ins = [soa(q, k) for k in ("Hd", "c", "A", "b", "lb", "ub")]

    def forward():
        sol = torch.full((3, B), 7.0, dtype=torch.float64, device=DEV)
        st = torch.zeros(B, dtype=torch.int32, device=DEV)
        it = torch.zeros(B, dtype=torch.int32, device=DEV)
        hip.qp_solve_batch(*ins, sol, st, iters=it)
        torch.cuda.synchronize()
        return sol, st, it

    before = forward()
    keep = [t.clone() for t in ins]
    rc = torch.zeros(B, dtype=torch.int32, device=DEV)
    hip.qp_vjp_batch(*ins, soa(q, "gsol"), rc, gA=torch.empty_like(ins[2]), gc=torch.empty_like(ins[1]))
    torch.cuda.synchronize()
    after = forward()
    for a, b in zip(before + tuple(keep), after + tuple(ins)):
        assert torch.equal(a, b)
    assert bool((rc == before[1]).all())
