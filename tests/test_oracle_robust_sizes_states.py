"""The state generator of tests/synth_robust_states.py, judged by the oracle alone: on its batches every reduced row
of the robust filter's QP decides answers, for every number of half-planes and every option set the GPU tests run."""
import numpy as np
import pytest

import synth_robust_states as S


@pytest.mark.parametrize("N", range(1, 9))
def test_every_row_binds_under_every_option_set(oracle, N):
    """For N half-planes and each option set: every row (s, p), s < N, binds (synth_robust_states.binding) on at least
    8 instances with rc = 1; for N >= 2 at least 20 instances have rc = -1; at least 64 have u* moved off clip(uDes);
    at least half the batch has rc = 1.

    Which placement of the facets: on a facet whose normal points into the second or fourth quadrant of the (angle,
    velocity) plane the drift alone points inwards (Lfh_s > 0) along its whole length, so the row of its pair that a
    HELPING u would make tight (hi for a_{s,1} > 0, lo for a_{s,1} < 0) binds only past the facet's ends, on a handful
    of states or none.  For N >= 2 the batches therefore come in two placements, PHASE and a quarter
    turn (and a tenth of a facet) on, and a row counts with the placement in which it binds more often -- it must reach
    8 in ONE of them; the other three conditions hold in each placement.  N = 1 uses the first placement alone."""
    fams = [S.family(oracle, N, ph) for ph in range(len(S.phases(N)))]
    for fam in fams:
        assert fam["x"].shape == (S.B, 2) and S.B <= 2048
        assert fam["dropped"] <= S.DROP_CAP * fam["drawn"], (fam["dropped"], fam["drawn"])
    for name in S.OPTION_SETS:
        counts = np.max([S.binding_counts(oracle, fam, name) for fam in fams], axis=0)
        print(f"N={N} {name}: rows binding (lo, hi) per s: " + " ".join(f"({a},{b})" for a, b in counts))
        assert counts.shape == (N, 2) and counts.min() >= 8, (name, counts.tolist())
        for fam in fams:
            s = fam["sets"][name]
            rc, o = s["rc"], s["o"]
            assert np.all((rc == 1) | (rc == -1))
            assert (rc == 1).sum() >= S.B // 2
            if N >= 2:
                assert (rc == -1).sum() >= 20, (name, fam["ph"], (rc == -1).sum())
            moved = (rc == 1) & (np.abs(s["ua"][:, 0] - np.clip(fam["udes"][:, 0], o.lb[0], o.ub[0])) > S.TIE)
            assert moved.sum() >= 64, (name, fam["ph"], moved.sum())
            assert np.all(np.isfinite(s["rl"][rc == 1])) and np.all(np.isnan(s["rl"][rc != 1]))


def test_option_sets_are_what_they_say(oracle):
    o = S.options(oracle, 7, "tight_box", S.phases(7)[1])
    assert (o.nHalfPlanes, o.lb[0], o.ub[0]) == (7, -0.3, 0.2)
    a = np.array(o.halfPlanes[:14]).reshape(7, 2)
    np.testing.assert_allclose(np.hypot(a[:, 0], a[:, 1]), 1 / np.pi, rtol=1e-15)
    assert tuple(o.halfPlanes[14:]) == S.STALE_SLOT and np.abs(a[:, 1]).min() > 1e-3
    o = S.options(oracle, 3, "zero_radius")
    assert o.pMin == o.pMax == 1.0
    o = S.options(oracle, 3, "relax")
    assert (o.relaxLb, o.relaxCost) == (0.0, 5.0)
    d = oracle.dims(S.MODEL, S.VARIANT, S.options(oracle, 5))
    assert (d.nv, d.nc) == (22, 15)
