"""The robust pendulum filter's fused path (k_robust.hip: robust_rows_small, RobustPolicy::load, launch_robust_ip) for
every safe-set size it carries, N = 1 ... 8 half-planes: the half branch (RobustPolicy<4>, N <= 4) and the full one
(RobustPolicy<8>, N = 5 ... 8), every lanes_per_qp, on states where every reduced row decides answers
(tests/synth_robust_states.py, whose coverage tests/test_oracle_robust_sizes_states.py proves on the CPU).  The
reference is the oracle's exact optimum of the same filter; nothing is excluded here."""
import numpy as np
import pytest
import torch

import synth_robust_states as S

pytestmark = pytest.mark.gpu
U_TOL = 1e-6      # the suite's bar on |u - u_ref|
D_RTOL = 1e-5     # relaxation: relative to max(1, |delta_ref|), as tests/test_gpu_qp_lds.py holds the lifted problem
U0, R0 = 7.0, -7.0
CASES = [(N, ph) for N in range(1, 9) for ph in range(len(S.phases(N)))]
_ids = lambda c: f"N{c[0]}-ph{c[1]}"
_worst = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _filter(hip, o, xs, us, lanes=0, flt=None):
    """One launch on SoA xs [2,B], us [1,B]; uact starts at U0, relax at R0."""
    own = flt is None
    if own:
        flt = hip.Filter(S.MODEL, S.VARIANT, options=o, solver=hip.default_solver(lanes_per_qp=lanes))
    d = flt.dims
    B = xs.shape[1]
    uact = torch.full((1, B), U0, dtype=torch.float64, device="cuda:0")
    relax = torch.full((1, B), R0, dtype=torch.float64, device="cuda:0")
    rc = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    diag = torch.full((d.ndiag, B), -1.0, dtype=torch.float64, device="cuda:0")
    flt.filter(_dev(xs), _dev(us), uact, relax, rc, diag)
    torch.cuda.synchronize()
    out = dict(uact=uact.cpu().numpy(), relax=relax.cpu().numpy(), rc=rc.cpu().numpy(), diag=diag.cpu().numpy(), dims=d)
    if own:
        flt.close()
    return out


def _assemble(hip, o, xs, flt=None):
    own = flt is None
    if own:
        flt = hip.Filter(S.MODEL, S.VARIANT, options=o)
    d = flt.dims
    B = xs.shape[1]
    A = torch.full((d.nc * d.nv, B), 3.0, dtype=torch.float64, device="cuda:0")
    b = torch.full((d.nc, B), 3.0, dtype=torch.float64, device="cuda:0")
    code = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    flt.assemble(_dev(xs), A, b, code, None)
    torch.cuda.synchronize()
    out = dict(A=A.cpu().numpy(), b=b.cpu().numpy(), code=code.cpu().numpy(), dims=d)
    if own:
        flt.close()
    return out


@pytest.mark.parametrize("name", list(S.OPTION_SETS))
@pytest.mark.parametrize("lanes", [2, 4, 8])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fused_filter_matches_exact_optimum(hip, oracle, case, lanes, name):
    """rc equal to the oracle's on every instance; |uact - u_ref| <= 1e-6 and |relax - delta_ref| <= 1e-5 max(1,
    |delta_ref|) where rc = 1; uact and relax untouched (7.0, -7.0) where it is not; lb <= uact <= ub exactly."""
    N, ph = case
    fam = S.family(oracle, N, ph)
    ref = fam["sets"][name]
    out = _filter(hip, S.options(hip, N, name, fam["phase"]), fam["xs"], fam["udes_s"], lanes)
    assert (out["dims"].nv, out["dims"].nc) == (2 + 4 * N, 3 * N)
    rc, ok = ref["rc"], ref["rc"] == 1
    du = np.abs(out["uact"][0, ok] - ref["ua"][ok, 0])
    dd = np.abs(out["relax"][0, ok] - ref["rl"][ok, 0]) / np.maximum(1.0, np.abs(ref["rl"][ok, 0]))
    w = _worst.setdefault(N, [0.0, 0.0])
    if np.array_equal(out["rc"], rc):
        w[0], w[1] = max(w[0], du.max()), max(w[1], dd.max())
    print(f"N={N} ph={ph} G={lanes} {name}: rc mismatches {(out['rc'] != rc).sum()}, max|u - u_ref| {du.max():.2e}, "
          f"max rel delta gap {dd.max():.2e}; worst so far for N={N}: {w[0]:.2e}, {w[1]:.2e}")
    assert np.array_equal(out["rc"], rc), f"rc mismatches {(out['rc'] != rc).sum()}"
    assert du.max() <= U_TOL
    assert dd.max() <= D_RTOL
    assert np.all(out["uact"][0, ~ok] == U0) and np.all(out["relax"][0, ~ok] == R0)
    o = ref["o"]
    assert np.all(out["uact"][0, ok] >= o.lb[0]) and np.all(out["uact"][0, ok] <= o.ub[0])
    it = out["diag"][-1]
    assert np.all(np.isfinite(it)) and np.all(it >= 0)


@pytest.mark.parametrize("name", S.PM_SETS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_assembled_rows_match_oracle(hip, oracle, case, name):
    """asif_hip_assemble_batch against oracle.assemble_batch on 512 of the generator's states: 3N x (2 + 4N), code 1,
    b bit-identical, A to rtol 1e-12 / atol 1e-13, the structural entries (0, +-1) exact."""
    N, ph = case
    fam = S.family(oracle, N, ph)
    n = 512
    out = _assemble(hip, S.options(hip, N, name, fam["phase"]), np.ascontiguousarray(fam["xs"][:, :n]))
    o = S.options(oracle, N, name, fam["phase"])
    A, b, code, _ = oracle.assemble_batch(S.MODEL, S.VARIANT, o, fam["x"][:n])
    nv, nc = 2 + 4 * N, 3 * N
    assert (out["dims"].nv, out["dims"].nc) == (nv, nc) and A.shape == (n, nv * nc)
    assert np.all(out["code"] == 1) and np.all(code == 1)
    assert np.array_equal(out["b"].T, b)
    np.testing.assert_allclose(out["A"].T, A, rtol=1e-12, atol=1e-13)
    interval = np.zeros((nv, nc), bool)  # [col, row]: h and the four interval ends of every safety row
    for s in range(N):
        interval[[1, 2 + 4 * s, 3 + 4 * s, 4 + 4 * s, 5 + 4 * s], 3 * s] = True
    structural = ~interval.reshape(-1)
    assert np.all(np.isin(A[:, structural], (0.0, 1.0, -1.0)))
    assert np.array_equal(out["A"].T[:, structural], A[:, structural])


# ------------------------------------------------------------------ launch-shape edges on the full branch: N = 7, G = 8
N_EDGE, G_EDGE = 7, 8


@pytest.fixture(scope="module")
def full_run(hip, oracle):
    fam = S.family(oracle, N_EDGE, 0)
    return fam, _filter(hip, S.options(hip, N_EDGE, "default", fam["phase"]), fam["xs"], fam["udes_s"], G_EDGE)


@pytest.mark.parametrize("B", [1, 7, 65])
def test_small_batches_in_padded_buffers(hip, full_run, B):
    """B instances in buffers of row stride B + 19: bit-equal to the same instances of the B = 2048 run, every column
    beyond B untouched."""
    fam, full = full_run
    ld = B + 19
    flt = hip.Filter(S.MODEL, S.VARIANT, options=S.options(hip, N_EDGE, "default", fam["phase"]),
                     solver=hip.default_solver(lanes_per_qp=G_EDGE))
    nd = flt.dims.ndiag
    rows = max(2, nd)
    # every tensor is a slice of a [rows, ld] buffer, so that all share the stride ld
    mk = lambda v, dt=torch.float64: torch.full((rows, ld), v, dtype=dt, device="cuda:0")
    x, u, uact, relax, diag = mk(1e300), mk(1e300), mk(U0), mk(R0), mk(-3.0)
    rc = torch.full((ld,), -77, dtype=torch.int32, device="cuda:0")
    x[:2, :B] = _dev(fam["xs"][:, :B])
    u[:1, :B] = _dev(fam["udes_s"][:, :B])
    flt.filter(x[:2, :B], u[:1, :B], uact[:1, :B], relax[:1, :B], rc[:B], diag[:nd, :B])
    torch.cuda.synchronize()
    flt.close()
    uact, relax, diag, rc = (t.cpu().numpy() for t in (uact, relax, diag, rc))
    assert np.array_equal(uact[0, :B], full["uact"][0, :B]) and np.array_equal(relax[0, :B], full["relax"][0, :B])
    assert np.array_equal(rc[:B], full["rc"][:B])
    assert np.array_equal(diag[nd - 1, :B], full["diag"][nd - 1, :B])
    assert np.all(uact[:, B:] == U0) and np.all(relax[:, B:] == R0) and np.all(rc[B:] == -77)
    assert np.all(diag[:, B:] == -3.0)
    assert np.all(uact[1:] == U0) and np.all(relax[1:] == R0) and np.all(diag[nd:] == -3.0)


def test_update_options_across_the_half_full_switch(hip, oracle):
    """update_options on a live handle, N = 4 -> 7 -> 2 -> 4: dims follow, filter and assemble outputs are bit-equal to
    a fresh handle's."""
    flt = hip.Filter(S.MODEL, S.VARIANT, options=S.options(hip, 4), solver=hip.default_solver(lanes_per_qp=G_EDGE))
    first = True
    for N in (4, 7, 2, 4):
        fam = S.family(oracle, N, 0)
        o = S.options(hip, N, "default", fam["phase"])
        if not first:
            flt.update_options(o)
        first = False
        assert (flt.dims.nv, flt.dims.nc, flt.dims.npSS) == (2 + 4 * N, 3 * N, N)
        xs, us = fam["xs"][:, :1024], fam["udes_s"][:, :1024]
        live, fresh = _filter(hip, o, xs, us, flt=flt), _filter(hip, o, xs, us, G_EDGE)
        for k in ("uact", "relax", "rc", "diag"):
            assert np.array_equal(live[k], fresh[k]), (N, k)
        ref = fam["sets"]["default"]
        assert np.array_equal(live["rc"], ref["rc"][:1024])
        live, fresh = _assemble(hip, o, xs, flt=flt), _assemble(hip, o, xs)
        for k in ("A", "b", "code"):
            assert np.array_equal(live[k], fresh[k]), (N, k)
        assert live["A"].shape[0] == (2 + 4 * N) * 3 * N
    flt.close()


@pytest.mark.parametrize("B, lanes", [(16384, 4), (8192, 8)])
def test_automatic_lane_choice(hip, oracle, B, lanes):
    """lanes_per_qp = 0 takes 4 lanes from 16 384 instances and 8 below (launch_robust_ip): bit-equal to asking."""
    fam = S.family(oracle, N_EDGE, 0)
    o = S.options(hip, N_EDGE, "default", fam["phase"])
    xs, us = np.tile(fam["xs"], (1, B // S.B)), np.tile(fam["udes_s"], (1, B // S.B))
    auto, asked = _filter(hip, o, xs, us, 0), _filter(hip, o, xs, us, lanes)
    for k in ("uact", "relax", "rc", "diag"):
        assert np.array_equal(auto[k], asked[k]), k
    assert np.array_equal(auto["rc"][:S.B], fam["sets"]["default"]["rc"])


def test_diag_holds_an_iteration_count(full_run):
    _, full = full_run
    it = full["diag"][-1]
    assert np.all(np.isfinite(it)) and np.all(it >= 0) and np.all(it == np.floor(it))
