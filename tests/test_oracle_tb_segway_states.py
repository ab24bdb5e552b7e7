"""tests/synth_states.py reaches what it is there for -- by the oracle alone, no GPU.

The seeded segway batch has idxHit = 1 on every instance that gets rows (4096 states: 47 with code 1, all at the first
step).  These are conditions on the INPUTS of tests/test_gpu_tb_segway_late.py: late hits past the first two blocks
of the trajectory (the sensitivity wave of the two-role pass runs one block behind), hits in the last block and on its
last sample, at a block's first and last sample, both branches of the hit scan's early exit, the three codes side by
side in every wave, short trajectories padded with inert rows next to long ones."""
import numpy as np
import pytest

import synth_states as S


@pytest.fixture(scope="module", params=["fine_step", "default"])
def fam(request, oracle):
    return S.late_hit_family(oracle, request.param)


def test_the_family_reaches_its_paths(fam, oracle):
    code, diag, npBT = fam["code"], fam["diag"], fam["npBT"]
    B = len(code)
    assert B <= 2048 and npBT == 316  # the default number of samples: the kernel's usual bound on the rows applies
    m = code == 1
    hit = diag[m, 2].astype(int)
    ortho = diag[m, 1]
    minOrtho = fam["o"].backTrajMinOrtho
    nblk = (npBT + S.BLOCK - 1) // S.BLOCK
    by_block = np.bincount(hit // S.BLOCK, minlength=nblk)
    print(f"\n{fam['name']}: codes " + ", ".join(f"{c}: {(code == c).sum()}" for c in (1, 2, -3)))
    print("idxHit by block of %d samples (block: count): " % S.BLOCK +
          " ".join(f"{k}:{n}" for k, n in enumerate(by_block) if n))
    print(f"ortho > 2 minOrtho: {(ortho > 2 * minOrtho).sum()}, ortho < minOrtho: {(ortho < minOrtho).sum()}, "
          f"idxHit < 3: {(hit < 3).sum()}, idxHit = npBT - 1: {(hit == npBT - 1).sum()}")
    assert m.sum() >= 256
    assert (hit >= 2 * S.BLOCK).sum() >= 128
    assert (hit >= (nblk - 1) * S.BLOCK).sum() >= 32 and (hit == npBT - 1).sum() >= 4
    assert (hit % S.BLOCK == 0).sum() >= 32 and (hit % S.BLOCK == S.BLOCK - 1).sum() >= 32
    assert np.count_nonzero(by_block) >= nblk - 1  # every block of the pass is some instance's last (block 0: samples 1-3)
    # both branches of `if (ortho > 2 * backTrajMinOrtho) break`, and hits kept below the orthogonality floor
    assert (ortho > 2 * minOrtho).sum() >= 32 and (ortho <= 2 * minOrtho).sum() >= 32
    assert (ortho < minOrtho).sum() >= 32
    # the three codes inside every span of 64 instances
    for s in range(0, B, 64):
        assert {1, 2, -3} <= set(code[s:s + 64].tolist()), s
    # fewer trajectory points than rows (inert padding) and more candidates than rows
    assert (hit + 1 < 4).sum() >= 8 and (hit + 1 > 4).sum() >= 128
    short = np.where(m)[0][hit + 1 < 4]
    assert np.all(fam["crit"][short, 3] == -1) and np.all(fam["A"][short].reshape(-1, 2, 18)[:, 1, 12:16] == 1.0)
    # critical samples beyond the first block, and not only the hit sample's own block
    crit = fam["crit"][m]
    assert (crit.max(axis=1) >= 2 * S.BLOCK).sum() >= 128
    assert (crit[:, 0] // S.BLOCK != hit // S.BLOCK).sum() >= 64
    # nothing within a rounding of another outcome (the generator's margins, re-read from the oracle)
    assert np.all(diag[m | (code == 2), 3] >= S.TIE_MARGIN) and np.all(diag[m | (code == -3), 4] <= -S.TIE_MARGIN)


def test_the_filter_sees_solved_failed_and_trivial_instances(fam, oracle):
    B = len(fam["code"])
    ua, rl, rc = oracle.filter_batch(S.MODEL, S.VARIANT, fam["o"], fam["x"], fam["udes"],
                                     uact_init=np.full((B, 1), 7.0))
    m = fam["code"] == 1
    print(f"\n{fam['name']}: rc " + ", ".join(f"{c}: {(rc == c).sum()}" for c in np.unique(rc)))
    assert np.array_equal(rc[~m], fam["code"][~m])
    assert (rc[m] == 1).sum() >= 128 and (rc[m] != 1).sum() >= 32
    late = fam["diag"][:, 2] >= 2 * S.BLOCK
    assert (m & late & (rc == 1)).sum() >= 64


def test_the_seeded_batch_never_hits_late(oracle):
    """What the family is for: on the seeded workload every instance with rows hits on its first step."""
    model, variant = oracle.CONFIGS[4]
    x, _ = oracle.make_batch(4, 2048)
    _, _, code, diag = oracle.assemble_batch(model, variant, oracle.default_options(model, variant), x)
    assert (code == 1).sum() >= 10 and np.all(diag[code == 1, 2] == 1)
