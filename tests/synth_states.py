"""Segway states for the time-to-backup-set filter that reach the backup set LATE, built by construction.

The seeded workload (workloads.make_batch(4, ...)) only ever produces rows for trajectories that enter the backup set
on their first Euler step, so nothing the kernel does beyond that step can change a compared number.  The states here
are made the other way round: a point just inside the backup set's boundary, taken k steps back along the closed-loop
backup flow (the inverse of the forward-Euler step, by fixed-point iteration on the oracle's own fCl), with k spread
over the whole trajectory.  The oracle then decides what each candidate is; candidates whose outcome hangs on a
rounding are left out HERE, on the CPU, so that no test excludes anything:

  * the backup-set function at the hit sample, at the start (code 2), and its closest approach to zero among the
    samples scanned before the hit (code -3: among all samples) must be at least TIE_MARGIN away from zero -- a hit one
    sample earlier or later is another idxHit, another code, another rc;
  * the rows must not move by more than ULP_RESPONSE x the comparison bound (rtol 1e-7, atol 1e-9) when every state
    component moves by one ulp.  The device differs from the oracle by contracted multiply-adds and its own sin / cos
    / tanh at each of up to 315 steps, i.e. by the equivalent of some hundreds of one-ulp perturbations along the
    trajectory; an instance that amplifies ONE ulp to a thousandth of the bound cannot be held to the bound (the hit
    grazes the set: the rows divide by grad hBS . fCl);
  * the QP must stay feasible / infeasible when its right-hand sides move by 1e-8 relative: rc 1 against -1.

Two named option sets.  "fine_step" keeps the default NUMBER of samples (316) at a fifth of the step, so the pitch moves
by less per step than the carried sin / cos accept (kTrigCarryMaxStep) on every trajectory: the kernel's fast, two-role
pass.  "default" is the example's options: the states that hit late there are fast ones, whose blocks the kernel
repeats on its checking step.  Everything is seeded; numpy and the oracle only, no GPU."""
import numpy as np

MODEL, VARIANT = 2, 2  # oracle_lib.MODEL_SEGWAY, VAR_TB (the same numbers in asif_amd.capi)
XB = np.array([3.0, 3.0, np.pi / 6, np.pi])  # examples/segway_implicit_tb.cpp: xBound
PV = 0.05                                    # backup set: Pv^2 - sum (x_i / xBound_i)^2 >= 0
BLOCK = 4                                    # Segway::kTrajBlock (asif_amd/csrc/models.hpp)

OPTION_SETS = {
    "fine_step": dict(backTrajDt=0.002, backTrajHorizon=0.6),
    "default": dict(),
}
TIE_MARGIN = 1e-10
ULP_RESPONSE = 1e-3
RTOL, ATOL = 1e-7, 1e-9  # the bound tests/test_gpu_tb.py holds this kernel's rows to


def options(lib, name):
    """The named option set on lib's defaults; lib is oracle_lib or asif_amd.capi (same field names)."""
    o = lib.default_options(MODEL, VARIANT)
    for k, v in OPTION_SETS[name].items():
        setattr(o, k, v)
    return o


def _steps_back(oracle, o, xk, k):
    """xk [n,4] taken k[n] forward-Euler steps back: y with y + dt fCl(y) = x, four fixed-point sweeps per step."""
    x = xk.copy()
    dt = o.backTrajDt
    for j in range(int(k.max())):
        a = k > j
        y = x[a]
        for _ in range(4):
            y = x[a] - dt * oracle.model_eval(MODEL, VARIANT, o, y)["fCl"]
        x[a] = y
    return x


def _candidates(oracle, o, n, rng):
    """n states meant to hit late, n / 4 inside the backup set, n / 4 scattered (mostly never reaching it)."""
    d = oracle.dims(MODEL, VARIANT, o)
    dirs = rng.standard_normal((3 * n, 4))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    xb = PV * XB * dirs  # on hBS = 0
    e = oracle.model_eval(MODEL, VARIANT, o, xb)
    inward = np.where((e["DhBS"] * e["fCl"]).sum(axis=1) > 0)[0][:n]
    xk = xb[inward] + (rng.uniform(0.1, 0.9, len(inward)) * o.backTrajDt)[:, None] * e["fCl"][inward]
    k = rng.integers(1, d.npBT, len(inward))
    # the ends of the trajectory by quota: the first samples (fewer trajectory points than rows), the last block
    q = len(inward) // 16
    k[:q] = rng.integers(1, 4, q)
    k[q:3 * q] = rng.integers(d.npBT - BLOCK, d.npBT, 2 * q)
    k[3 * q:4 * q] = d.npBT - 1
    late = _steps_back(oracle, o, xk, k)
    late = late[np.all(np.isfinite(late), axis=1)]
    inside = PV * XB * dirs[-(n // 4):] * rng.uniform(0.0, 0.97, (n // 4, 1))
    far = XB * rng.uniform(-1.0, 1.0, (n // 4, 4)) * np.array([0.3, 0.5, 1.0, 1.0])
    return np.concatenate([late, inside, far])


def _well_posed(oracle, o, x, A, b, code, diag):
    ok = np.ones(len(x), bool)
    ok &= ~((code == 1) | (code == 2)) | (diag[:, 3] >= TIE_MARGIN)
    ok &= ~((code == 1) | (code == -3)) | (diag[:, 4] <= -TIE_MARGIN)
    sgn = np.where(np.arange(4) % 2 == 0, 1.0, -1.0)
    for s in (sgn, -sgn):
        Ap, bp, cp, dp = oracle.assemble_batch(MODEL, VARIANT, o, np.nextafter(x, s * np.inf))
        ok &= (cp == code) & (dp[:, 2] == diag[:, 2])
        m = code == 1
        moved = np.maximum((np.abs(Ap - A) / (ATOL + RTOL * np.abs(A))).max(axis=1),
                           (np.abs(bp - b) / (ATOL + RTOL * np.abs(b))).max(axis=1))
        ok &= ~m | (moved <= ULP_RESPONSE)
    # feasibility of the 2 x 18 QP away from its edge (uDes does not enter it)
    m = np.where(code == 1)[0]
    Hd, c, lb, ub, _ = oracle.qp_static(MODEL, VARIANT, o, np.zeros(1))
    tile = lambda v: np.tile(v, (len(m), 1))
    st = []
    for s in (1.0, -1.0):
        bs = b[m] + s * 1e-8 * (1.0 + np.abs(b[m]))
        st.append(oracle.qp_solve_batch(2, 18, tile(Hd), tile(c), A[m], bs, tile(lb), tile(ub),
                                        solver=oracle.SOLVER_EXACT)[1])
    ok[m] &= st[0] == st[1]
    return ok


_cache = {}


def late_hit_family(oracle, name="fine_step", B=2048, seed=20240):
    """dict(x [B,4], udes [B,1] AoS; xs [4,B], udes_s [1,B] SoA for the device; o: the oracle's options; A, b, code,
    diag: oracle.assemble_batch on x; crit [B,4]: the critical sample indexes, -1 where the trajectory is shorter).
    Half the batch has code 1, the rest is split between 2 and -3, shuffled so that every span of 64 mixes them."""
    key = (name, B, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    o = options(oracle, name)
    x = _candidates(oracle, o, 2 * B, rng)
    A, b, code, diag = oracle.assemble_batch(MODEL, VARIANT, o, x)
    ok = _well_posed(oracle, o, x, A, b, code, diag)
    want = {1: B - 2 * (B // 4), 2: B // 4, -3: B // 4}
    pick = []
    for c, n in want.items():
        i = np.where(ok & (code == c))[0]
        assert len(i) >= n, (name, c, len(i), n)
        pick.append(i[:n] if c != 1 else i[np.sort(rng.permutation(len(i))[:n])])
    pick = np.concatenate(pick)[rng.permutation(B)]
    x = np.ascontiguousarray(x[pick])
    udes = rng.uniform(-25.0, 25.0, (B, 1))
    crit = np.full((B, 4), -1, dtype=np.int64)
    for i in np.where(code[pick] == 1)[0]:
        oracle.assemble(MODEL, VARIANT, o, x[i])
        ci = oracle.last_crit_idx()
        crit[i, :len(ci)] = ci
    fam = dict(name=name, o=o, x=x, udes=udes, xs=np.ascontiguousarray(x.T), udes_s=np.ascontiguousarray(udes.T),
               A=A[pick], b=b[pick], code=code[pick], diag=diag[pick], crit=crit,
               npBT=oracle.dims(MODEL, VARIANT, o).npBT)
    for k, v in fam.items():
        if isinstance(v, np.ndarray) and k not in ("xs", "udes_s"):  # (torch warns about read-only arrays)
            v.setflags(write=False)
    _cache[key] = fam
    return fam
