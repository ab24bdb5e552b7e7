"""The two data-driven filters (k_realizable.hip, k_robust_data.hip) on data the reference does not ship: the
synthetic polytopes and half-plane sets of tests/synth_kernels.py, whose coverage tests/test_oracle_synth_kernels.py
pins on the CPU.  Every comparison is against the oracle at the bars of the shipped-data tests: rows, codes and index
lists identical, rc identical, |u - u_ref| and |relax - relax_ref| <= 1e-6 where rc == 1, outputs untouched elsewhere.

What runs here and nowhere else in the suite: the scalar-load facet scan (more than 768 facets, both row counts),
facet counts below four and not a multiple of four, eight critical facets kept and a ninth dropped, one and two
active constraints per facet, axis-aligned facets, exact ties in h, four-wave workgroups of this class, ragged and
padded batches without diagnostics; for the half-plane filter npSSmax == N, npSSmax defaulted, N below the group
width, N not a multiple of it, N = 1000, duplicated rows, ragged and padded batches."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth_kernels as S

pytestmark = pytest.mark.gpu
UACT0, RELAX0 = 7.0, -7.0


def _t(a):
    return np.ascontiguousarray(a.T)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _filter(flt, x, u, diag=True):
    d, B = flt.dims, x.shape[1]
    uact = torch.full((d.nu, B), UACT0, dtype=torch.float64, device="cuda:0")
    relax = torch.full((d.nrelax, B), RELAX0, dtype=torch.float64, device="cuda:0")
    rc = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    dg = torch.zeros((d.ndiag, B), dtype=torch.float64, device="cuda:0") if diag else None
    flt.filter(_dev(x), _dev(u), uact, relax, rc, dg)
    torch.cuda.synchronize()
    return dict(uact=uact.cpu().numpy(), relax=relax.cpu().numpy(), rc=rc.cpu().numpy(),
                diag=dg.cpu().numpy() if diag else None)


def _assemble(flt, x, diag=True, keep=None):
    d, B = flt.dims, x.shape[1]
    A = torch.zeros((d.nc * d.nv, B), dtype=torch.float64, device="cuda:0")
    b = torch.zeros((d.nc, B), dtype=torch.float64, device="cuda:0")
    code = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    dg = torch.zeros((d.ndiag, B), dtype=torch.float64, device="cuda:0") if diag else None
    flt.assemble(_dev(x), A, b, code, dg)
    torch.cuda.synchronize()
    n = B if keep is None else keep
    return dict(A=A[:, :n].cpu().numpy(), b=b[:, :n].cpu().numpy(), code=code[:n].cpu().numpy(),
                diag=dg[:, :n].cpu().numpy() if diag else None)


def _same_lists(got, want, what):
    """Index lists [B, n] identical on every instance; a failure names how many differ and the first that does."""
    bad = np.where((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.shape[0]} instances differ, first at {bad[0]}: "
                           f"device {got[bad[0]].tolist()}, oracle {want[bad[0]].tolist()}")


def _check_filter(out, ref, B):
    """out: device, ref: the oracle's (uact [B,nu], relax [B,nrelax], rc)."""
    ua, rl, rc = ref
    assert np.array_equal(out["rc"], rc), f"rc mismatches {(out['rc'] != rc).sum()} of {B}"
    ok = rc == 1
    if ok.any():
        assert np.abs(out["uact"][:, ok] - ua[ok].T).max() <= 1e-6
        assert np.abs(out["relax"][:, ok] - rl[ok].T).max() <= 1e-6
    assert np.all(out["uact"][:, ~ok] == UACT0) and np.all(out["relax"][:, ~ok] == RELAX0)


def _dims(hip, flt):
    """The handle's dimensions as the library reports them now (not the Python object's copy)."""
    d = hip.Dims()
    hip.check(flt.lib.asif_hip_get_dims(flt.handle, C.byref(d)))
    return d


def _check_padded_calls(hip, flt, x, u, ref):
    """Both C entries with ld = B + 59 and diag == NULL: inputs beyond B hold 1e9, outputs beyond B must keep their
    marker, and inside B the results are the dense call's bits (which in turn meet the oracle's `ref`)."""
    B = x.shape[1]
    d, ld = flt.dims, B + 59
    dense, rows = _filter(flt, x, u, diag=False), _assemble(flt, x, diag=False)
    _check_filter(dense, ref, B)
    dev = "cuda:0"
    tx = torch.full((d.nx, ld), 1e9, dtype=torch.float64, device=dev)
    tu = torch.full((d.nu, ld), 1e9, dtype=torch.float64, device=dev)
    tx[:, :B], tu[:, :B] = _dev(x), _dev(u)
    uact = torch.full((d.nu, ld), -5.0, dtype=torch.float64, device=dev)
    relax = torch.full((d.nrelax, ld), -5.0, dtype=torch.float64, device=dev)
    rc = torch.full((ld,), 77, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    hip.check(flt.lib.asif_hip_filter_batch(flt.handle, B, ld, p(tx), p(tu), p(uact), p(relax), p(rc), None, None))
    A = torch.full((d.nc * d.nv, ld), -5.0, dtype=torch.float64, device=dev)
    b = torch.full((d.nc, ld), -5.0, dtype=torch.float64, device=dev)
    code = torch.full((ld,), 77, dtype=torch.int32, device=dev)
    hip.check(flt.lib.asif_hip_assemble_batch(flt.handle, B, ld, p(tx), p(A), p(b), p(code), None, None))
    torch.cuda.synchronize()
    assert np.array_equal(rc[:B].cpu().numpy(), dense["rc"])
    ok = dense["rc"] == 1
    assert np.array_equal(uact[:, :B].cpu().numpy()[:, ok], dense["uact"][:, ok])
    assert np.array_equal(relax[:, :B].cpu().numpy()[:, ok], dense["relax"][:, ok])
    assert torch.all(uact[:, :B][:, _dev(~ok)] == -5.0) and torch.all(relax[:, :B][:, _dev(~ok)] == -5.0)
    assert np.array_equal(A[:, :B].cpu().numpy(), rows["A"]) and np.array_equal(b[:, :B].cpu().numpy(), rows["b"])
    assert np.array_equal(code[:B].cpu().numpy(), rows["code"])
    assert torch.all(rc[B:] == 77) and torch.all(uact[:, B:] == -5.0) and torch.all(relax[:, B:] == -5.0)
    assert torch.all(code[B:] == 77) and torch.all(A[:, B:] == -5.0) and torch.all(b[:, B:] == -5.0)


# ------------------------------------------------------------------------------------------------ realizable
def _rz_check_lists(diag, info, z):
    """nCrit, the critical facets and the barrier facets of the diagnostics against the oracle's info."""
    assert np.array_equal(diag[0].astype(np.int32), info[:, 0])
    _same_lists(diag[1:1 + z.maxCrit].T.astype(np.int32), info[:, 1:1 + z.maxCrit], "critical facets")
    _same_lists(diag[1 + z.maxCrit:1 + z.maxCrit + z.npSSmax].T.astype(np.int32), info[:, 1 + z.maxCrit:],
                "barrier facets")


def _rz_against_oracle(hip, oracle, k, x, u, **kw):
    """One kernel polytope, both entries, against the oracle; returns (oracle handle, info, rc) for further checks."""
    okw = dict(kw)
    if "uncertaintyBounds" in kw:
        kw = dict(kw, uncertaintyBounds=list(kw["uncertaintyBounds"]) + [0.0, 0.0])
    flt = hip.RealizableFilter(k, options=hip.default_realizable_options(**kw))
    z = oracle.Realizable(k, **okw)
    assert (flt.dims.nv, flt.dims.nc, flt.dims.ndiag) == (z.nv, z.nc, 1 + z.maxCrit + z.npSSmax + 1)
    rows = _assemble(flt, x)
    A, b, code, info = z.assemble(_t(x))
    assert np.array_equal(rows["code"], code)
    _rz_check_lists(rows["diag"], info, z)
    assert np.array_equal(rows["A"].T, A)
    assert np.array_equal(rows["b"].T, b)
    out = _filter(flt, x, u)
    ref = z.filter(_t(x), _t(u))
    _check_filter(out, ref, x.shape[1])
    _rz_check_lists(out["diag"], info, z)
    flt.close()
    return z, info, ref[2]


@pytest.mark.parametrize("npSSmax", [2, 3])
def test_square_on_the_exact_lattice(hip, oracle, npSSmax):
    """Axis-aligned facets (one extent exactly zero) and exact ties in h, on states where nothing rounds: which
    facets touch, and which facet wins a tie, cannot be blamed on rounding.  npSSmax 2 and 3 are the two select
    networks (KB == 2, KB == 4)."""
    from asif_amd import workloads
    k = S.square()
    x = S.lattice()
    B = x.shape[1]
    u = (-20.0 + 40.0 * workloads.uniform(61, np.arange(B, dtype=np.uint64), 2))[None, :]
    z, info, rc = _rz_against_oracle(hip, oracle, k, x, u, npSSmax=npSSmax, uncertaintyBounds=S.SQUARE_UNC)
    # the project's rule, stated without the oracle: smallest h first, lowest facet index on ties
    h = S.margins(k["facetNormals"], x)
    order = np.argsort(h, axis=1, kind="stable")[:, :npSSmax]
    hs = np.sort(h, axis=1)
    tied = (hs[:, 0] == hs[:, 1]) | (hs[:, 1] == hs[:, 2])
    assert tied.sum() >= 100
    assert np.array_equal(info[tied, 1 + z.maxCrit:], order[tied])
    assert (rc[tied] == 1).sum() >= 20  # tied states whose barrier rows reach the solve


@pytest.mark.parametrize("n,maxCrit,nA", S.NGON_SMALL)
def test_small_and_odd_facet_counts(hip, oracle, n, maxCrit, nA):
    """nF < 4 (the unrolled-by-four scan never runs), nF % 4 in {1, 3}, one and two active constraints per facet."""
    from asif_amd import workloads
    k = S.ngon(n, maxCrit, nA)
    x, u = workloads.make_batch_realizable(k, 2048)
    _rz_against_oracle(hip, oracle, k, x, u)


@pytest.mark.parametrize("case", ["801", "1000"])
def test_more_than_768_facets(hip, oracle, case):
    """The scalar-load form of the facet scan, realizable_filter_kernel<2, false> and <4, false>.  The 801-gon with
    the wide uncertainty box is also the "eight kept, ninth dropped" case (both 64-bit index words full)."""
    from asif_amd import workloads
    if case == "801":
        k, kw = S.ngon(**S.NGON_801), dict(npSSmax=2, uncertaintyBounds=S.NGON_801_UNC)
    else:
        k, kw = S.ngon(**S.NGON_1000), dict(npSSmax=4)
    assert k["facetVertices"].shape[0] * 64 > 48 * 1024
    x, u = workloads.make_batch_realizable(k, 2048)
    z, info, rc = _rz_against_oracle(hip, oracle, k, x, u, **kw)
    if case == "801":
        assert (info[:, 0] == 8).sum() >= 500


@pytest.mark.parametrize("name", ["square", "ngon5", "ngon801"])
def test_device_tables_match_oracle_tables(hip, oracle, name):
    k = {"square": S.square, "ngon5": lambda: S.ngon(5, 5, 3), "ngon801": lambda: S.ngon(**S.NGON_801)}[name]()
    flt = hip.RealizableFilter(k)
    table, bbox = flt.tables()
    t, bb = oracle.Realizable(k).table()
    assert table.shape == (k["facetVertices"].shape[0], k["maxActiveConstraints"], 4)
    assert np.array_equal(table, t)
    assert np.array_equal(bbox, bb)
    flt.close()


@pytest.mark.parametrize("B", [1, 65, 257])
def test_ragged_padded_and_no_diag(hip, oracle, B):
    """ld > B and diag == NULL through the C entries: nothing beyond B is read into a result or written, and the
    first B results are the dense call's bits."""
    from asif_amd import workloads
    k = S.ngon(7, 8, 2)
    x, u = workloads.make_batch_realizable(k, B)
    flt = hip.RealizableFilter(k)
    z = oracle.Realizable(k)
    _check_padded_calls(hip, flt, x, u, z.filter(_t(x), _t(u)))
    flt.close()


@pytest.mark.parametrize("name", ["100Hz", "ngon801"])
def test_a_batch_equals_the_prefix_of_a_larger_one(hip, name):
    """Device against device: 1000 instances alone (one-wave workgroups) and as the first 1000 of a ragged batch large
    enough for four-wave workgroups (which share one LDS copy of the facet records where it fits)."""
    from asif_amd import workloads
    if name == "100Hz":
        k, o = workloads.load_kernel("100Hz"), None
    else:
        k = S.ngon(**S.NGON_801)
        o = hip.default_realizable_options(uncertaintyBounds=list(S.NGON_801_UNC) + [0.0, 0.0])
    n = 1000
    big = 2 * 64 * torch.cuda.get_device_properties(0).multi_processor_count + 4099
    x, u = workloads.make_batch_realizable(k, big)
    flt = hip.RealizableFilter(k, options=o)
    small, large = _filter(flt, x[:, :n], u[:, :n]), _filter(flt, x, u)
    for key in ("uact", "relax", "rc", "diag"):
        assert np.array_equal(small[key], large[key][..., :n]), key
    assert (small["rc"] == 1).sum() > n // 2 and (small["diag"][0] > 0).sum() > n // 10
    rs, rl = _assemble(flt, x[:, :n]), _assemble(flt, x, keep=n)
    for key in ("A", "b", "code", "diag"):
        assert np.array_equal(rs[key], rl[key]), key
    flt.close()


def test_limits_are_refused_cleanly(hip, oracle):
    """npSSmax == nFacets (the reference's unsorted branch) is refused by design, and so are more facets than a
    16-bit index holds; neither leaves the process unable to build the next filter."""
    from asif_amd import workloads
    for k, m in ((S.ngon(3, 3, 1), 3), (S.square(), 4), (S.ngon(3, 3, 1), 4)):
        with pytest.raises(hip.AsifHipError):
            hip.RealizableFilter(k, options=hip.default_realizable_options(npSSmax=m))
    with pytest.raises(hip.AsifHipError):
        hip.RealizableFilter(S.ngon(65536, 3, 1))
    flt = hip.RealizableFilter(S.ngon(5, 5, 3))
    with pytest.raises(hip.AsifHipError):  # refused update: the handle keeps its options
        flt.update_options(hip.default_realizable_options(npSSmax=5))
    assert _dims(hip, flt).nc == 3 * 15 + 2 and _dims(hip, flt).ndiag == 1 + 5 + 2 + 1
    flt.close()
    k = S.ngon(5, 5, 3)
    x, u = workloads.make_batch_realizable(k, 256)
    _rz_against_oracle(hip, oracle, k, x, u)


# ---------------------------------------------------------------------------------------------- robust data
def _rb_check_rows(flt, z, x):
    rows = _assemble(flt, x)
    A, b, code, sel = z.assemble(_t(x))
    M = z.npSSmax
    assert np.array_equal(rows["code"], code)
    _same_lists(rows["diag"][:M].T.astype(np.int32), sel, "kept half-planes (rows kernel)")
    assert np.array_equal(rows["A"].T, A) and np.array_equal(rows["b"].T, b)
    return sel


@pytest.fixture(scope="module")
def rb_refs(oracle):
    """Oracle results per (N, npSSmax), computed once and shared by the three group widths."""
    from asif_amd import workloads
    refs = {}

    def get(N, npSSmax, duplicates=0, B=1024):
        key = (N, npSSmax, duplicates, B)
        if key not in refs:
            hp = S.halfplanes(N, S.rb_seed(N), duplicates)
            x, u = workloads.make_batch_robust_data(hp, B)
            z = oracle.RobustData(hp, npSSmax=npSSmax)
            ref = z.filter(_t(x), _t(u))
            for a in ref:
                a.setflags(write=False)
            refs[key] = (hp, x, u, z, ref, z.assemble(_t(x))[3])
        return refs[key]
    return get


@pytest.mark.parametrize("lanes", [2, 4, 8])
@pytest.mark.parametrize("N,npSSmax", S.RB_CASES)
def test_small_and_large_sets(hip, rb_refs, N, npSSmax, lanes):
    """npSSmax == N (rows in data order), npSSmax > N (defaulted to N), N below the group width (lanes without a
    half-plane), N not a multiple of it, and a scan a hundred deep per lane."""
    hp, x, u, z, ref, sel = rb_refs(N, npSSmax)
    flt = hip.RobustDataFilter(hp, options=hip.default_robust_data_options(npSSmax=npSSmax),
                               solver=hip.default_solver(lanes_per_qp=lanes))
    assert (flt.dims.nv, flt.dims.nc, flt.dims.nrelax) == (z.nv, z.nc, 1)
    out = _filter(flt, x, u)
    _check_filter(out, ref, x.shape[1])
    _same_lists(out["diag"][:z.npSSmax].T.astype(np.int32), sel, "kept half-planes (fused kernel)")
    if lanes == 2:  # the rows kernel does not depend on the group width
        _rb_check_rows(flt, z, x)
    flt.close()


@pytest.mark.parametrize("lanes", [2, 4, 8])
def test_duplicate_half_planes(hip, rb_refs, lanes):
    """Equal margins in different lanes of a group: the head extraction must take the lowest index first."""
    d = S.RB_DUP
    hp, x, u, z, ref, sel = rb_refs(d["N"], d["npSSmax"], d["duplicates"])
    flt = hip.RobustDataFilter(hp, options=hip.default_robust_data_options(npSSmax=d["npSSmax"]),
                               solver=hip.default_solver(lanes_per_qp=lanes))
    out = _filter(flt, x, u)
    _same_lists(out["diag"][:z.npSSmax].T.astype(np.int32), sel, "kept half-planes (fused kernel)")
    _check_filter(out, ref, x.shape[1])
    _rb_check_rows(flt, z, x)
    flt.close()


def test_update_options_changes_the_row_count(hip, oracle):
    from asif_amd import workloads
    N = 13
    hp = S.halfplanes(N, S.rb_seed(N))
    x, u = workloads.make_batch_robust_data(hp, 1024)
    flt = hip.RobustDataFilter(hp, options=hip.default_robust_data_options(npSSmax=5))

    def same_as_fresh_oracle(M):
        z = oracle.RobustData(hp, npSSmax=M)
        d = _dims(hip, flt)
        assert (d.nv, d.nc, d.ndiag) == (2 + 4 * M, 3 * M, M + 1)
        _check_filter(_filter(flt, x, u), z.filter(_t(x), _t(u)), x.shape[1])
        _rb_check_rows(flt, z, x)

    same_as_fresh_oracle(5)
    flt.update_options(hip.default_robust_data_options(npSSmax=8))
    same_as_fresh_oracle(8)
    with pytest.raises(hip.AsifHipError):  # -1 means "all N rows": 13 > 8 rows is more than the QP kernels hold
        flt.update_options(hip.default_robust_data_options(npSSmax=-1))
    assert flt.options.npSSmax == 8
    same_as_fresh_oracle(8)  # the refused update left the handle as it was
    flt.close()


@pytest.mark.parametrize("lanes", [2, 4, 8])
@pytest.mark.parametrize("B", [1, 7, 65])
def test_ragged_and_padded(hip, oracle, B, lanes):
    from asif_amd import workloads
    N = 9
    hp = S.halfplanes(N, S.rb_seed(N))
    x, u = workloads.make_batch_robust_data(hp, B)
    flt = hip.RobustDataFilter(hp, options=hip.default_robust_data_options(npSSmax=8),
                               solver=hip.default_solver(lanes_per_qp=lanes))
    z = oracle.RobustData(hp, npSSmax=8)
    _check_padded_calls(hip, flt, x, u, z.filter(_t(x), _t(u)))
    flt.close()
