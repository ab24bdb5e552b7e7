"""Segway time-to-backup-set filter on states that reach the backup set LATE (tests/synth_states.py).

The seeded batch only produces rows for trajectories that hit on their first Euler step; on it nothing the kernel does
beyond that step -- the segway Jacobian in the sensitivity, the sensitivity wave running a block behind, the carried
sin / cos, the checkpoints and the re-integration of a block other than the first, the selection among more than two
samples -- can change a compared bit.  Here idxHit is spread over all 79 blocks of the pass (by the oracle alone:
tests/test_oracle_tb_segway_states.py).  Two option sets, both with the default 316 samples, so the rows are held to
the bound of tests/test_gpu_tb.py: "fine_step" keeps every trajectory on the fast two-role pass, "default" has the late
hits on states whose blocks are repeated on the checking step.  Measured on an MI355X: worst relative gap of the rows
5.0e-11 (fine_step) and 2.0e-10 (default), 0.05 % and 0.3 % of the bound; codes, idxHit, critical samples and rc equal.

The generator leaves out, on the CPU, every state whose outcome hangs on a rounding; no test here excludes anything."""
import numpy as np
import pytest
import torch

import gpu_util
import synth_states as S

pytestmark = pytest.mark.gpu
NAMES = ["fine_step", "default"]


@pytest.fixture(scope="module", params=NAMES)
def fam(request, oracle):
    return S.late_hit_family(oracle, request.param)


def _oracle_filter(oracle, fam, sel=slice(None), uact_init=7.0, relax_init=-7.0):
    x, udes = fam["x"][sel], fam["udes"][sel]
    ua, rl, rc = oracle.filter_batch(S.MODEL, S.VARIANT, fam["o"], x, udes, uact_init=np.full((len(x), 1), uact_init))
    return ua.T, np.where(np.isnan(rl), relax_init, rl).T, rc


def test_rows_codes_and_diagnostics(hip, oracle, fam):
    out = gpu_util.run_assemble(4, 0, options=S.options(hip, fam["name"]), x=fam["xs"])
    assert out["dims"].npBT == fam["npBT"] == 316
    code, diag = fam["code"], fam["diag"]
    assert np.array_equal(out["code"], code), f"{(out['code'] != code).sum()} codes differ"
    m = code == 1
    assert np.array_equal(out["diag"][2][m], diag[m, 2]), "idxHit"
    assert np.array_equal(out["diag"][3:7].T[m].astype(np.int64), fam["crit"][m]), "critical samples"
    for k in ("A", "b"):
        got, want = out[k].T[m], fam[k][m]
        gap = np.abs(got - want) / (S.ATOL + S.RTOL * np.abs(want))
        rel = (np.abs(got - want) / np.maximum(np.abs(want), 1e-300))[np.abs(want) > 1e-2].max()
        print(f"\n{fam['name']} {k}: worst gap {gap.max():.3g} of the bound, worst relative gap {rel:.3g}")
    np.testing.assert_allclose(out["A"].T[m], fam["A"][m], rtol=S.RTOL, atol=S.ATOL)
    np.testing.assert_allclose(out["b"].T[m], fam["b"][m], rtol=S.RTOL, atol=S.ATOL)
    t = code == 2
    assert np.all(out["A"].T[t] == 0.0) and np.all(out["b"].T[t] == -1e20)
    np.testing.assert_allclose(out["diag"][0][m], diag[m, 0], rtol=1e-12)  # TTS_
    np.testing.assert_allclose(out["diag"][1][m], diag[m, 1], rtol=1e-8)   # BTorthoBS_
    assert np.all(out["diag"][1][t] == 1.0) and np.all(out["diag"][1][code == -3] == 0.0)


@pytest.mark.parametrize("lanes", [0, 2, 4])
def test_filter_matches_exact_optimum(hip, oracle, fam, lanes):
    """lanes 0: the default mode (the rows kernel solves the QP itself); 2 and 4: rows kernel + stage 2."""
    s = hip.default_solver(lanes_per_qp=lanes) if lanes else None
    out = gpu_util.run_filter(4, 0, solver=s, options=S.options(hip, fam["name"]), x=fam["xs"], udes=fam["udes_s"],
                              uact_init=7.0, relax_init=-7.0)
    ua, rl, rc = _oracle_filter(oracle, fam)
    assert np.array_equal(out["rc"], rc), f"rc mismatches {(out['rc'] != rc).sum()}"
    assert np.abs(out["uact"] - ua).max() <= 1e-6
    ok = (rc == 1) | (rc == 2)
    assert np.abs(out["relax"][:, ok] - rl[:, ok]).max() <= 1e-6
    assert np.all(out["relax"][:, ~ok] == -7.0)


def _save(fam, tmp_path, B):
    p = str(tmp_path / "late.npz")
    np.savez(p, xs=np.ascontiguousarray(fam["xs"][:, :B]), udes_s=np.ascontiguousarray(fam["udes_s"][:, :B]))
    return ("import synth_states as S\nd = np.load(%r); o = S.options(capi, %r)\n" % (p, fam["name"]) +
            "r = gpu_util.run_assemble(4, 0, options=o, x=d['xs'])\n"
            "f = gpu_util.run_filter(4, 0, options=o, x=d['xs'], udes=d['udes_s'], uact_init=7.0, relax_init=-7.0)\n")


def test_two_role_pass_is_bitwise_the_fused_pass(hip, oracle, tmp_path):
    """ASIF_HIP_TB_SPLIT 1 / 0, each in a process of its own, on a ragged batch of the fine-step family: the x wave and
    the sensitivity wave a block behind it against one wave doing both, on trajectories hundreds of blocks long."""
    body = _save(S.late_hit_family(oracle, "fine_step"), tmp_path, 2003)
    res = [gpu_util.child_digests(body, {"ASIF_HIP_TB_SPLIT": v}, timeout=300) for v in ("1", "0")]
    assert res[0] == res[1]


def test_one_two_and_four_waves_per_workgroup_give_the_same_bits(hip, oracle, tmp_path):
    body = _save(S.late_hit_family(oracle, "fine_step"), tmp_path, 2003)
    one, two, four = (gpu_util.child_digests(body, {"ASIF_HIP_WG_WAVES": v}, timeout=300) for v in ("1", "2", "4"))
    assert one == four == two


def test_fused_solve_and_its_hand_over_to_stage_two(hip, fam, monkeypatch):
    """ASIF_HIP_TB_FUSE unset / 0 / 2 / 3 (tests/test_gpu_tb.py), on QPs that come out of long trajectories."""
    outs = []
    for v in (None, "0", "2", "3"):
        if v is None:
            monkeypatch.delenv("ASIF_HIP_TB_FUSE", raising=False)
        else:
            monkeypatch.setenv("ASIF_HIP_TB_FUSE", v)
        outs.append(gpu_util.run_filter(4, 0, options=S.options(hip, fam["name"]), x=fam["xs"], udes=fam["udes_s"],
                                        uact_init=7.0, relax_init=-7.0))
    ref = outs[0]
    assert {1, 2, -3} <= set(np.unique(ref["rc"]).tolist())
    for o in outs[1:]:
        assert np.array_equal(o["rc"], ref["rc"]) and np.array_equal(o["uact"], ref["uact"])
        assert np.array_equal(o["relax"], ref["relax"]) and np.array_equal(o["diag"], ref["diag"])


def test_the_batch_equals_the_prefix_of_one_that_takes_the_other_layout(hip, fam):
    """Up to two waves per CU (32 768 instances on 256 CUs) launch_tb runs the two-role pass, or the fused pass with
    the checkpoints in an LDS region of their own; one wave more and it is the fused pass on the spilling layout in
    four-wave workgroups.  The family alone against the family at the head of 32 768 + 64 instances, the rest seeded."""
    from asif_amd import workloads
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = 2 * cus * 64 + 64
    n = fam["xs"].shape[1]
    px, pu = workloads.make_batch(4, big - n)
    xs, us = np.concatenate([fam["xs"], px], axis=1), np.concatenate([fam["udes_s"], pu], axis=1)
    o = S.options(hip, fam["name"])
    small = gpu_util.run_filter(4, 0, options=o, x=fam["xs"], udes=fam["udes_s"], uact_init=3.0)
    large = gpu_util.run_filter(4, 0, options=o, x=xs, udes=us, uact_init=3.0)
    for k in ("uact", "relax", "rc"):
        assert np.array_equal(small[k], large[k][..., :n], equal_nan=True), k
    rs, rl = gpu_util.run_assemble(4, 0, options=o, x=fam["xs"]), gpu_util.run_assemble(4, 0, options=o, x=xs)
    for k in ("A", "b", "code", "diag"):
        assert np.array_equal(rs[k], rl[k][..., :n], equal_nan=True), k


@pytest.mark.parametrize("B", [1, 63, 65, 1000])
def test_small_and_ragged_batches(hip, oracle, fam, B):
    """The head of the family against the oracle, and bit for bit what the same instances get in the full batch where
    their wave is the same 64 instances (a partial wave may take the checking step where the full one does not)."""
    sel = slice(0, B)
    out = gpu_util.run_filter(4, 0, options=S.options(hip, fam["name"]), x=np.ascontiguousarray(fam["xs"][:, sel]),
                              udes=np.ascontiguousarray(fam["udes_s"][:, sel]), uact_init=7.0, relax_init=-7.0)
    ua, rl, rc = _oracle_filter(oracle, fam, sel)
    assert np.array_equal(out["rc"], rc)
    assert np.abs(out["uact"] - ua).max() <= 1e-6
    full = gpu_util.run_filter(4, 0, options=S.options(hip, fam["name"]), x=fam["xs"], udes=fam["udes_s"],
                               uact_init=7.0, relax_init=-7.0)
    whole = B // 64 * 64
    for k in ("uact", "relax", "rc"):
        assert np.array_equal(out[k][..., :whole], full[k][..., :whole]), k
    assert np.array_equal(out["rc"], full["rc"][:B])
    assert np.abs(out["uact"] - full["uact"][:, :B]).max() <= 1e-10


def test_a_nan_state_among_late_hits(hip, oracle, fam):
    """One NaN state in a wave of late-hit instances: its rc is the oracle's, the wave's other lanes move by rounding at
    most (their blocks are repeated on the checking step), every other wave not at all (tests/test_gpu_nonfinite.py)."""
    o = S.options(hip, fam["name"])
    late = np.where((fam["code"] == 1) & (fam["diag"][:, 2] >= 2 * S.BLOCK))[0]
    bad = int(late[late >= 64][0])  # not in the first wave
    x = fam["xs"].copy()
    x[2, bad] = np.nan
    clean = gpu_util.run_filter(4, 0, options=o, x=fam["xs"], udes=fam["udes_s"], uact_init=7.0, relax_init=-7.0)
    out = gpu_util.run_filter(4, 0, options=o, x=x, udes=fam["udes_s"], uact_init=7.0, relax_init=-7.0)
    xb = fam["x"][bad:bad + 1].copy()
    xb[0, 2] = np.nan
    _, _, rcb = oracle.filter_batch(S.MODEL, S.VARIANT, fam["o"], xb, fam["udes"][bad:bad + 1],
                                    uact_init=np.full((1, 1), 7.0))
    assert out["rc"][bad] == rcb[0] and rcb[0] not in (1, 2)
    keep = np.ones(x.shape[1], bool)
    keep[bad] = False
    assert np.array_equal(out["rc"][keep], clean["rc"][keep])
    wave = np.zeros_like(keep)
    wave[bad // 64 * 64:bad // 64 * 64 + 64] = True
    for k in ("uact", "relax"):
        assert np.abs(out[k][..., keep] - clean[k][..., keep]).max() <= 1e-10, k
        assert np.array_equal(out[k][..., ~wave], clean[k][..., ~wave]), k


def test_a_handle_created_with_the_option_set(hip, oracle):
    """The fine-step set through asif_hip_create and through asif_hip_update_options on a default handle.  The second
    sizes the trajectory without the (1 + backTrajExtend) factor (src/asif_implicit_tb.cpp:377): 301 samples, so the
    hits past sample 300 become code -3 and the others keep their code and idxHit."""
    fam = S.late_hit_family(oracle, "fine_step")
    o = S.options(hip, "fine_step")
    flt = hip.Filter(hip.MODEL_SEGWAY, hip.IMPLICIT_TB, options=o)
    assert flt.dims.npBT == 316
    flt.close()
    flt = hip.Filter(hip.MODEL_SEGWAY, hip.IMPLICIT_TB)
    flt.update_options(o)
    assert flt.dims.npBT == 301
    n = 256
    dev = torch.device("cuda:0")
    tx = torch.from_numpy(np.ascontiguousarray(fam["xs"][:, :n])).to(dev)
    A = torch.zeros((36, n), dtype=torch.float64, device=dev)
    b = torch.zeros((18, n), dtype=torch.float64, device=dev)
    code = torch.zeros(n, dtype=torch.int32, device=dev)
    diag = torch.zeros((flt.dims.ndiag, n), dtype=torch.float64, device=dev)
    flt.assemble(tx, A, b, code, diag)
    torch.cuda.synchronize()
    flt.close()
    hit = fam["diag"][:n, 2]
    want = np.where((fam["code"][:n] == 1) & (hit > 300), -3, fam["code"][:n])
    assert (want != fam["code"][:n]).sum() >= 4
    assert np.array_equal(code.cpu().numpy(), want)
    m = want == 1
    assert np.array_equal(diag[2].cpu().numpy()[m], hit[m])
