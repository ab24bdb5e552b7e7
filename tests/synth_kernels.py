"""Synthetic data for the two data-driven filter classes: kernel polytopes for ASIFrealizable and half-plane
sets for ASIFrobust, generated (numpy only, no GPU, no oracle) so that the suite can reach the shapes the shipped
data never has -- three facets, more than 768, axis-aligned facets, exact ties in h, 1 to 1000 half-planes,
duplicated rows.  tests/test_oracle_synth_kernels.py checks on the CPU that every family exercises what it is
there for; tests/test_gpu_synth_kernels.py compares the device against the oracle on them."""
import numpy as np


def polygon_kernel(vertices, maxCriticalFacets, maxActiveConstraints):
    """Kernel dict (capi.RealizableFilter / oracle_lib.Realizable) of a convex polygon around the origin given by
    its vertices in order.  Facet i joins vertex i and vertex i+1; its normal n_i is scaled so that n_i . x == 1 on
    the facet (h_i = 1 - n_i . x > 0 inside); its active constraints are the nA facets i, i+1, ..."""
    V = np.ascontiguousarray(vertices, dtype=np.float64)
    nF, nA = V.shape[0], int(maxActiveConstraints)
    assert V.shape == (nF, 2) and nF >= 3 and 1 <= nA <= nF
    i = np.arange(nF)
    FV = np.stack([i, (i + 1) % nF], axis=1).astype(np.int32)
    v0, v1 = V[FV[:, 0]], V[FV[:, 1]]
    det = v0[:, 0] * v1[:, 1] - v0[:, 1] * v1[:, 0]  # twice the area of (0, v0, v1): non-zero around the origin
    assert np.all(det > 0) or np.all(det < 0), "vertices must go around the origin one way"
    N = np.stack([(v1[:, 1] - v0[:, 1]) / det, (v0[:, 0] - v1[:, 0]) / det], axis=1)
    FA = np.stack([(i + k) % nF for k in range(nA)], axis=1).astype(np.int32)
    return dict(vertices=V, facetVertices=FV, facetNormals=np.ascontiguousarray(N), facetActive=FA,
                maxCriticalFacets=int(maxCriticalFacets), maxActiveConstraints=nA)


def square(maxCriticalFacets=4, maxActiveConstraints=2):
    """Vertices (+-2, +-2): normals (+-0.5, 0), (0, +-0.5), every number dyadic, every facet axis-aligned."""
    return polygon_kernel([[2.0, 2.0], [-2.0, 2.0], [-2.0, -2.0], [2.0, -2.0]], maxCriticalFacets,
                          maxActiveConstraints)


def ngon(n, maxCriticalFacets=3, maxActiveConstraints=3):
    """An ellipse of radii 3 and 2.5 sampled at n equal angles."""
    t = 2.0 * np.pi * np.arange(n) / n
    return polygon_kernel(np.stack([3.0 * np.cos(t), 2.5 * np.sin(t)], axis=1), maxCriticalFacets,
                          maxActiveConstraints)


def lattice(step=1.0 / 8, half_width=2.5):
    """All states (a, b) of the grid of that step over [-half_width, half_width]^2, SoA [2, B] (41 x 41 = 1681 with
    the defaults).  On square() with uncertainty bounds (0.25, 0.25) every quantity of the facet scan -- h, the
    bounding-box prefilter, both touch tests -- is a small dyadic number: nothing rounds, on either side."""
    m = int(round(half_width / step))
    g = np.arange(-m, m + 1) * step
    a, b = np.meshgrid(g, g, indexing="ij")
    return np.ascontiguousarray(np.stack([a.ravel(), b.ravel()]))


def halfplanes(N, seed, duplicates=0):
    """[N, 2] rows a_i of half-planes a_i . x <= 1 at distance 1/|a_i| in [1.5, 2.5] from the origin, at sorted
    random angles; the last `duplicates` rows are exact copies of the first ones."""
    assert 0 <= duplicates and 2 * duplicates <= N
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, N))
    dist = rng.uniform(1.5, 2.5, N)
    hp = np.stack([np.cos(ang) / dist, np.sin(ang) / dist], axis=1)
    if duplicates:
        hp[N - duplicates:] = hp[:duplicates]
    return np.ascontiguousarray(hp)


def margins(normals, x):
    """h [B, nF] as both the device and the oracle round it: h = 1; h -= n_0 x_0; h -= n_1 x_1.  x is SoA [2, B]."""
    h = np.ones((x.shape[1], normals.shape[0]))
    h -= normals[None, :, 0] * x[0][:, None]
    h -= normals[None, :, 1] * x[1][:, None]
    return h


def touching_facets(kernel, x, unc):
    """For every state, the facets whose segment meets the box [x - unc, x + unc], decided from the vertex data in
    exact rational arithmetic (fractions of the float64 values), independent of the oracle and of the device.
    x is SoA [2, B]; returns a list of index lists in facet order."""
    from fractions import Fraction as Fr
    V, FV = kernel["vertices"], kernel["facetVertices"]
    out = []
    for k in range(x.shape[1]):
        hit = []
        for f in range(FV.shape[0]):
            p, q = V[FV[f, 0]], V[FV[f, 1]]
            lo, hi, ok = Fr(0), Fr(1), True  # the parameters t of p + t (q - p) inside the box
            for c in range(2):
                a, d = Fr(float(p[c])), Fr(float(q[c])) - Fr(float(p[c]))
                l, u = Fr(float(x[c, k])) - Fr(float(unc[c])) - a, Fr(float(x[c, k])) + Fr(float(unc[c])) - a
                if d == 0:
                    ok = ok and l <= 0 <= u
                else:
                    t0, t1 = sorted((l / d, u / d))
                    lo, hi = max(lo, t0), min(hi, t1)
            if ok and lo <= hi:
                hit.append(f)
        out.append(hit)
    return out


# ---- the cases both test files run (the CPU file checks that they exercise their paths, the GPU file runs them)
SQUARE_UNC = (0.25, 0.25)
NGON_SMALL = [(3, 3, 1), (5, 5, 3), (7, 8, 2)]  # (n, maxCriticalFacets, maxActiveConstraints)
NGON_801 = dict(n=801, maxCriticalFacets=8, maxActiveConstraints=2)  # scalar-load scan, KB = 2, eight kept
NGON_801_UNC = (0.1, 0.1)
NGON_1000 = dict(n=1000, maxCriticalFacets=3, maxActiveConstraints=3)  # scalar-load scan, KB = 4
RB_CASES = [(1, 1), (3, 3), (5, 8), (8, 8), (9, 8), (13, 5), (1000, 8)]  # (N, npSSmax)
RB_DUP = dict(N=12, npSSmax=5, duplicates=4)


def rb_seed(N):
    return 100 + N
