"""CPU checks, on the oracle alone, that every synthetic family of tests/synth_kernels.py exercises what it is there
for: ties, full critical lists, all three return codes, selections in data order.  These are conditions on the
inputs of tests/test_gpu_synth_kernels.py, not measurements: an edit of a generator that quietly turned one of
those GPU tests into a no-op fails here.  Every number is a lower bound on what the generators gave when the
families were laid down (quoted next to each)."""
import numpy as np
import pytest

import synth_kernels as S


def _t(a):
    return np.ascontiguousarray(a.T)


def _counts(rc):
    return [int((rc == v).sum()) for v in (1, -1, -2)]


def _udes(B, seed):
    from asif_amd import workloads
    return (-20.0 + 40.0 * workloads.uniform(seed, np.arange(B, dtype=np.uint64), 2))[None, :]


def test_generators_are_what_they_say():
    k = S.square()
    assert np.array_equal(k["facetNormals"], [[0.0, 0.5], [-0.5, 0.0], [0.0, -0.5], [0.5, 0.0]])
    assert k["facetActive"].tolist() == [[0, 1], [1, 2], [2, 3], [3, 0]]
    assert k["facetVertices"].tolist() == [[0, 1], [1, 2], [2, 3], [3, 0]]
    x = S.lattice()
    assert x.shape == (2, 41 * 41) and np.array_equal(np.unique(x[0]), np.arange(-20, 21) / 8.0)
    for n in (3, 7, 801):
        k = S.ngon(n)
        v = k["vertices"][k["facetVertices"]]  # n . x == 1 at both ends of every facet, h > 0 at the origin
        assert np.abs(np.einsum("fk,fvk->fv", k["facetNormals"], v) - 1.0).max() <= 1e-12
        assert np.abs((k["vertices"] / [3.0, 2.5]) ** 2 @ [1.0, 1.0] - 1.0).max() <= 1e-12
    hp = S.halfplanes(12, 5, duplicates=4)
    d = 1.0 / np.hypot(hp[:, 0], hp[:, 1])
    assert d.min() >= 1.5 - 1e-12 and d.max() <= 2.5 + 1e-12
    assert np.array_equal(hp[8:], hp[:4]) and np.all(np.diff(np.arctan2(hp[:8, 1], hp[:8, 0]) % (2 * np.pi)) > 0)
    assert np.array_equal(hp, S.halfplanes(12, 5, duplicates=4)) and not np.array_equal(hp[:8], S.halfplanes(12, 6)[:8])


def test_square_on_the_lattice_has_ties_touches_and_every_return_code(oracle):
    """observed: 312 codes -1; nCrit 1 on 540 states, 2 on 100; rc 1 / -1 / -2 = 999 / 370 / 312; 81 and 81 ties"""
    k = S.square()
    x = S.lattice()
    z = oracle.Realizable(k, npSSmax=2, uncertaintyBounds=S.SQUARE_UNC)
    _, _, code, info = z.assemble(_t(x))
    _, _, rc = z.filter(_t(x), _t(_udes(x.shape[1], 61)))
    assert (code == -1).sum() >= 200
    assert (info[:, 0] == 1).sum() >= 300 and (info[:, 0] == 2).sum() >= 50
    h = np.sort(S.margins(k["facetNormals"], x), axis=1)
    assert (h[:, 0] == h[:, 1]).sum() >= 50
    assert (h[:, 1] == h[:, 2]).sum() >= 50
    assert min(_counts(rc)) >= 100, _counts(rc)
    # the lattice is exact for this polytope: the touching facets follow from the vertex data alone
    sub = np.arange(0, x.shape[1], 7)
    for i, hit in zip(sub, S.touching_facets(k, x[:, sub], S.SQUARE_UNC)):
        assert hit == [f for f in info[i, 1:1 + z.maxCrit] if f >= 0]


def test_ngon_801_fills_the_critical_list_and_drops_a_ninth(oracle):
    """observed: 1089 instances at nCrit == 8; rc 1 / -1 / -2 = 1617 / 203 / 228"""
    from asif_amd import workloads
    k = S.ngon(**S.NGON_801)
    assert k["facetVertices"].shape[0] * 64 > 48 * 1024  # beyond the LDS copy of the facet records
    B = 2048
    x, u = workloads.make_batch_realizable(k, B)
    z = oracle.Realizable(k, npSSmax=2, uncertaintyBounds=S.NGON_801_UNC)
    _, _, _, info = z.assemble(_t(x))
    _, _, rc = z.filter(_t(x), _t(u))
    n = np.bincount(info[:, 0], minlength=9)
    assert n[8] >= 500 and n[5] >= 1 and n[6] >= 1 and n[7] >= 1, n
    c = _counts(rc)
    assert c[0] > B // 2 and c[1] >= 100 and c[2] >= 100, c
    # a ninth touching facet, from the vertex data and not from the oracle
    full = np.where(info[:, 0] == 8)[0][:8]
    hits = S.touching_facets(k, x[:, full], S.NGON_801_UNC)
    assert any(len(h) >= 9 for h in hits)
    for i, h in zip(full, hits):
        assert h[:8] == info[i, 1:9].tolist()  # "the first maxCrit in facet order"


def test_ngon_1000_reaches_the_four_row_kernel(oracle):
    """observed: nCrit 0..3 on 1330 / 36 / 89 / 593; rc 1 / -1 / -2 = 1483 / 112 / 453"""
    from asif_amd import workloads
    k = S.ngon(**S.NGON_1000)
    x, u = workloads.make_batch_realizable(k, 2048)
    z = oracle.Realizable(k, npSSmax=4)
    _, _, _, info = z.assemble(_t(x))
    _, _, rc = z.filter(_t(x), _t(u))
    assert (z.npSSmax, z.nc) == (4, 3 * 9 + 4) and (info[:, 0] == 3).sum() >= 300
    assert min(_counts(rc)) >= 100, _counts(rc)


@pytest.mark.parametrize("n,maxCrit,nA", S.NGON_SMALL)
def test_small_polygons_give_every_return_code(oracle, n, maxCrit, nA):
    """observed rc 1 / -1 / -2: 1034 / 331 / 683 (n = 3), 1039 / 520 / 489 (5), 1234 / 326 / 488 (7)"""
    from asif_amd import workloads
    k = S.ngon(n, maxCrit, nA)
    x, u = workloads.make_batch_realizable(k, 2048)
    z = oracle.Realizable(k)
    assert (z.npSS, z.nv, z.nc) == (maxCrit * nA, 1 + 4 * maxCrit * nA + 1, 3 * maxCrit * nA + 2)
    _, _, rc = z.filter(_t(x), _t(u))
    assert min(_counts(rc)) >= 100, _counts(rc)


@pytest.mark.parametrize("N,npSSmax", S.RB_CASES)
def test_half_plane_sets(oracle, N, npSSmax):
    """observed rc 1 / -1: 950 / 74, 841 / 183, 787 / 237, 743 / 281, 864 / 160, 909 / 115, 787 / 237"""
    from asif_amd import workloads
    hp = S.halfplanes(N, S.rb_seed(N))
    x, u = workloads.make_batch_robust_data(hp, 1024)
    z = oracle.RobustData(hp, npSSmax=npSSmax)
    M = min(npSSmax, N)
    assert (z.nv, z.nc, z.npSSmax) == (2 + 4 * M, 3 * M, M)
    _, _, code, sel = z.assemble(_t(x))
    _, _, rc = z.filter(_t(x), _t(u))
    assert (rc == 1).sum() >= 500 and (rc == -1).sum() >= 50 and np.all(code == 1)
    if npSSmax >= N:
        assert np.array_equal(sel, np.tile(np.arange(N, dtype=np.int32), (1024, 1)))
    else:
        h = 1.0 - hp[:, 0][None, :] * x[0][:, None] - hp[:, 1][None, :] * x[1][:, None]
        assert np.array_equal(sel, np.argsort(h, axis=1, kind="stable")[:, :M])


def test_duplicated_half_planes_are_kept_in_pairs(oracle):
    """observed: 771 of 1024 kept lists hold a row and its copy"""
    from asif_amd import workloads
    d = S.RB_DUP
    hp = S.halfplanes(d["N"], S.rb_seed(d["N"]), d["duplicates"])
    x, _ = workloads.make_batch_robust_data(hp, 1024)
    z = oracle.RobustData(hp, npSSmax=d["npSSmax"])
    _, _, _, sel = z.assemble(_t(x))
    first = d["N"] - d["duplicates"]
    n = 0
    for s in sel.tolist():
        pairs = [i for i in range(d["duplicates"]) if i in s and first + i in s]
        n += bool(pairs)
        for i in pairs:  # equal margins: the lower index first, its copy right behind it
            assert s.index(first + i) == s.index(i) + 1
    assert n >= 100
