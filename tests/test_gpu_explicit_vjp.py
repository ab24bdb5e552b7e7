"""asif_hip_filter_vjp_batch (asif_amd/csrc/k_explicit_vjp.hip) and the torch layer on top of it, against the numpy adjoint
of tests/vjp_ref.py (itself checked against finite differences of the oracle in tests/test_vjp_ref_host.py).

Parity bound per gradient entry: 1e-9 (1 + |ref|) max(1, 1 / sigma_min(G_W)).  The solution parity of this path is
3e-13; a gradient is a rational function of u* and the rows with conditioning 1 / sigma_min; a wrong working set is an
O(1) error.  Instances the reference flags degenerate (a second constraint within 1e-5, a multiplier below 1e-6,
|W| > nu) have a one-sided derivative and are skipped: at most 1 % of a batch, and every working-set size stays covered.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib
import vjp_ref
from asif_amd import workloads

pytestmark = pytest.mark.gpu

B = 2048
DEV = "cuda:0"
KEYS = ("gudes", "glfh", "glgh", "gx")


@functools.lru_cache(maxsize=None)
def case(cfg, lie, keep=0):
    """Inputs (SoA numpy) and the reference of one batch; computed once, shared, never written to."""
    oracle_lib.build()
    x, udes = workloads.make_batch(cfg, B)
    d = oracle_lib.dims(*oracle_lib.CONFIGS[cfg], oracle_lib.default_options(*oracle_lib.CONFIGS[cfg]))
    nc = keep if keep else d.nc
    rng = np.random.default_rng(cfg)
    lfh, lgh = rng.normal(0, 1, (nc, B)), rng.normal(0, 1, (nc * d.nu, B))
    gbar = rng.normal(0, 1, (d.nu, B))
    lies = (lfh, lgh) if lie else None
    ref = vjp_ref.vjp(oracle_lib, cfg, x, udes, gbar, lies, keep)
    for a in (x, udes, lfh, lgh, gbar, *ref.values()):
        a.setflags(write=False)
    return dict(cfg=cfg, x=x, udes=udes, lie=lies, gbar=gbar, ref=ref, keep=keep)


def make_filter(hip, cfg, keep=0, **solver):
    od = hip.default_options(*hip.CONFIGS[cfg][:2])
    od.npSSmax = keep
    return hip.Filter(*hip.CONFIGS[cfg][:2], options=od, solver=hip.default_solver(**solver) if solver else None)


def run_vjp(flt, c, n=B, ld=None, sentinel=0.0):
    """One filter_vjp call on the first n instances of case c in buffers of leading dimension ld, pre-filled with
    `sentinel`; returns the whole buffers."""
    ld = ld or n
    d = flt.dims

    def up(a):
        t = torch.full((a.shape[0], ld), sentinel, dtype=torch.float64, device=DEV)
        t[:, :n] = torch.from_numpy(np.array(a[:, :n]))  # a copy: the shared inputs are read-only
        return t

    def out(rows):
        return torch.full((rows, ld), sentinel, dtype=torch.float64, device=DEV)

    x, udes, gbar = up(c["x"]), up(c["udes"]), up(c["gbar"])
    res = dict(gudes=out(d.nu), rc=torch.full((ld,), -77, dtype=torch.int32, device=DEV))
    lfh = lgh = None
    if c["lie"] is not None:
        lfh, lgh = up(c["lie"][0]), up(c["lie"][1])
        res.update(glfh=out(d.nc), glgh=out(d.nc * d.nu), gx=out(d.nx))
    v = lambda t: None if t is None else t[..., :n]  # shape [rows, n], stride ld
    flt.filter_vjp(v(x), v(udes), v(gbar), v(res["gudes"]), res["rc"], v(lfh), v(lgh), v(res.get("glfh")),
                   v(res.get("glgh")), v(res.get("gx")))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in res.items()}


def check_parity(got, c):
    ref = c["ref"]
    assert np.array_equal(got["rc"], ref["rc"]), f"{(got['rc'] != ref['rc']).sum()} rc mismatches"
    ok = ref["rc"] == 1
    good = ok & ~ref["degenerate"]
    assert (ok & ref["degenerate"]).sum() <= 0.01 * B
    assert set(ref["nactive"][good]) == set(ref["nactive"][ok]) and len(set(ref["nactive"][good])) >= 2
    scale = np.maximum(1.0, 1.0 / ref["smin"])
    keys = KEYS if c["lie"] is not None else KEYS[:1]
    for k in keys:
        assert np.all(got[k][:, ~ok] == 0.0), f"{k}: a failed instance holds a gradient"
        gap = np.abs(got[k] - ref[k]) / ((1.0 + np.abs(ref[k])) * scale[None, :])
        worst = float(gap[:, good].max())
        print(f"cfg {c['cfg']} lie={c['lie'] is not None} keep={c['keep']} {k}: max scaled gap {worst:.3e}")
        assert worst <= 1e-9, (k, worst, int(np.argmax(gap[:, good].max(axis=0))))
    if c["lie"] is not None:  # rows outside the working set: exactly zero
        for k in ("glfh", "glgh"):
            assert np.all(got[k][:, good][ref[k][:, good] == 0.0] == 0.0)


@pytest.mark.parametrize("cfg,lie", [(2, False), (2, True), (11, False), (11, True)])
def test_parity(hip, cfg, lie):
    c = case(cfg, lie)
    ok = c["ref"]["rc"] == 1
    assert 1266 <= ok.sum() <= 1597 and 451 <= (~ok).sum() <= 782
    flt = make_filter(hip, cfg)
    check_parity(run_vjp(flt, c), c)
    flt.close()


@pytest.mark.parametrize("cfg,keep", [(2, 2), (11, 3)])
def test_row_selection(hip, cfg, keep):
    """npSSmax < npSS: the rows are the `keep` smallest h in ascending order, lfh / lgh and their gradients are indexed
    by that position; a dropped safety function has no slot and adds nothing to gx."""
    c = case(cfg, True, keep)
    flt = make_filter(hip, cfg, keep)
    assert flt.dims.nc == keep
    got = run_vjp(flt, c)
    assert got["glfh"].shape[0] == keep
    check_parity(got, c)
    flt.close()


def test_tail_and_leading_dimension(hip):
    c = case(11, True)
    flt = make_filter(hip, 11)
    full = run_vjp(flt, c)
    for n in (67, 1):
        got = run_vjp(flt, c, n=n, ld=128, sentinel=-3.25)
        for k in KEYS:
            assert np.all(got[k][:, n:] == -3.25), f"{k}: slots >= B written"
            assert np.array_equal(got[k][:, :n], full[k][:, :n]), f"{k}: differs from the B = {B} run"
        assert np.all(got["rc"][n:] == -77) and np.array_equal(got["rc"][:n], full["rc"][:n])
    flt.close()


def test_autograd_layer(hip):
    from asif_amd.torch_layer import ExplicitSafetyLayer
    c = case(11, True)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    layer = ExplicitSafetyLayer(hip.MODEL_PLANAR_TWO_INPUT)
    x, udes, lfh, lgh = (t(a).requires_grad_() for a in (c["x"], c["udes"], *c["lie"]))
    prev = torch.full((2, B), 0.125, dtype=torch.float64, device=DEV).requires_grad_()
    gbar = t(c["gbar"])
    uact, rc = layer(x, udes, lfh, lgh, uact_prev=prev)
    assert not rc.requires_grad
    (uact * gbar).sum().backward()
    torch.cuda.synchronize()

    direct = run_vjp(layer.filter, c)
    for ten, k in ((udes, "gudes"), (lfh, "glfh"), (lgh, "glgh"), (x, "gx")):
        assert np.array_equal(ten.grad.cpu().numpy(), direct[k]), k
    failed = direct["rc"] < 0
    assert np.array_equal(prev.grad.cpu().numpy(), np.where(failed[None, :], c["gbar"], 0.0))

    ua = torch.full((2, B), 0.125, dtype=torch.float64, device=DEV)
    relax = torch.zeros((1, B), dtype=torch.float64, device=DEV)
    rc2 = torch.zeros(B, dtype=torch.int32, device=DEV)
    layer.filter.filter_lie(x.detach(), udes.detach(), lfh.detach(), lgh.detach(), ua, relax, rc2)
    assert torch.equal(uact.detach(), ua) and torch.equal(rc, rc2)

    with pytest.raises(RuntimeError, match="second derivatives"):
        layer(t(c["x"]).requires_grad_(), t(c["udes"]))
    u2, _ = layer(t(c["x"]), t(c["udes"]).requires_grad_())  # the model path without a state gradient works
    assert u2.requires_grad


def test_contract(hip):
    lib = hip.load()
    n = 8
    buf = [torch.zeros((10, n), dtype=torch.float64, device=DEV) for _ in range(9)]
    rc = torch.zeros(n, dtype=torch.int32, device=DEV)
    p = [C.c_void_p(b.data_ptr()) for b in buf]
    prc = C.c_void_p(rc.data_ptr())

    def call(flt, nb, lfh, lgh, glfh=None, glgh=None, gx=None):
        return lib.asif_hip_filter_vjp_batch(flt.handle, nb, n, p[0], p[1], lfh, lgh, p[4], p[5], glfh, glgh, gx, prc,
                                             None)

    EINVAL, EUNSUPPORTED = -1, -3
    imp = hip.Filter(*hip.CONFIGS[3][:2])
    assert call(imp, n, None, None) == EUNSUPPORTED
    imp.close()
    flt = make_filter(hip, 2)
    assert call(flt, n, p[2], None) == EINVAL
    assert call(flt, n, None, p[3]) == EINVAL
    assert call(flt, n, None, None, glfh=p[6]) == EINVAL
    assert call(flt, n, None, None, gx=p[8]) == EINVAL
    assert call(flt, 0, None, None) == 0
    assert call(flt, n, None, None) == 0 and call(flt, n, p[2], p[3], p[6], p[7], p[8]) == 0
    torch.cuda.synchronize()
    flt.close()
    pol = make_filter(hip, 2, polish=1)
    assert call(pol, n, None, None) == EUNSUPPORTED
    pol.close()
    pre = make_filter(hip, 2, presolve=1)
    assert call(pre, n, None, None) == 0
    torch.cuda.synchronize()
    pre.close()


def test_forward_untouched(hip):
    c = case(2, False)
    flt = make_filter(hip, 2)
    x, udes = (torch.from_numpy(np.array(a)).to(DEV) for a in (c["x"], c["udes"]))

    def forward():
        ua = torch.full((1, B), 7.0, dtype=torch.float64, device=DEV)
        rl = torch.full((1, B), -7.0, dtype=torch.float64, device=DEV)
        rc = torch.zeros(B, dtype=torch.int32, device=DEV)
        flt.filter(x, udes, ua, rl, rc)
        torch.cuda.synchronize()
        return ua, rl, rc

    before = forward()
    run_vjp(flt, c)
    after = forward()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    flt.close()
