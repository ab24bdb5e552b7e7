"""States for the robust pendulum filter (BASELINE's C5 class) on safe sets of N = 1 ... 8 half-planes, built so that
every reduced row of the filter's 2-variable QP decides some instance's answer.

The safe set is 1 - a_k . x >= 0 with a_k = (cos, sin)(2 pi (k + PHASE) / N) / pi: N facets tangent to the circle of
radius pi (as in tests/test_gpu_qp_lds.py::_robust_qps_with_n_halfplanes, PHASE = 0.25).  After the multipliers are eliminated the filter
solves, per instance,

    min (u - uDes)^2 + relaxCost (delta - relaxLb)^2
    s.t.  lo(Lgh_s) u + h_s delta >= -lo(Lfh_s),   hi(Lgh_s) u + h_s delta >= -lo(Lfh_s),   s < N,
          lb <= u <= ub,  delta >= relaxLb,

rows r = 2 s + p.  Of a pair only the "lo" row (p = 0) can be the tighter one where u > 0 and only the "hi" row (p = 1)
where u < 0, so a row (s, p) BINDS on an instance when the filter answered (rc = 1), the row is tight at the optimum,
u* has the sign that makes it the tighter one of its pair, and the optimum is not the unconstrained one: u* off
clip(uDes) or delta* above relaxLb.  An implementation that dropped or misplaced that row answers differently there.

The seeded C5 states ([-3, 3]^2) leave whole rows unexamined -- the facets sit at distance pi, outside that square but
for its corners.  A batch of B = 2048 therefore mixes

  * N_SEEDED seeded C5 states with their uDes;
  * for every option set and every row (s, p), states AIMED at an optimum where that row alone is active (_aimed: the
    state is drawn in a band inside facet s, uDes is put 0.02 ... 0.6 beyond the u* the row allows, on the side it
    pushes back from), kept where the oracle confirms that the row binds there;
  * states scattered on each facet's line, up to half a facet length beyond its ends, and moved off it along the normal
    by 0.01 ... 0.35 to either side (just inside, just outside) or 0.35 ... 1.2 inside, with uDes in +-[0.05, 1.5]
    (the default input box), both signs in equal parts.

Not every row can bind in one placement of the polygon: where the drift alone keeps the state inside a facet (Lfh_s > 0
along the facet, as on the facets whose normal points into the second or fourth quadrant of the (angle, velocity)
plane), the row of its pair that a helping u would make tight never is.  phases(N) gives two placements, a quarter turn
apart; tests/test_oracle_robust_sizes_states.py requires every row to bind in one of them.  The half-plane slots from N
on hold STALE_SLOT, a half-plane most of these states violate: the filter must not read them, the oracle does not.

Instances whose verdict hangs on a rounding are left out HERE, on the CPU, so that no test excludes anything; two
cases, both judged by the oracle on the reduced QP under every option set of OPTION_SETS:

  * two candidate optima within TIE: the optimum sits at a point where more constraints are tight than it has variables
    (rows with identical coefficients counted once), i.e. two working sets of the oracle's enumeration give optima
    closer than TIE, and which of them an active-set method ends on is decided by the last bits of the rows;
  * an infeasibility margin within TIE: the oracle's verdict (solved / infeasible) changes when every right-hand side
    moves by TIE (1 + |b|) to one side or the other.

At most DROP_CAP of the B + B / 64 candidates drawn may go that way (family() asserts it).  Everything is seeded; numpy and the oracle only, no GPU."""
import numpy as np

MODEL, VARIANT = 3, 3  # oracle_lib.MODEL_IP_ROBUST, VAR_ROBUST (the same numbers in asif_amd.capi)
PHASE = 0.25


def phases(N):
    """The placements of the facets: PHASE and, for N >= 2, the same polygon a quarter turn and a tenth of a facet
    on (the tenth keeps every a_{s,1}, and with it Lgh_s, away from zero for every N).  For N = 1 the first placement
    lets both rows bind."""
    return (PHASE,) if N == 1 else (PHASE, PHASE + N / 4.0 + 0.1)


B = 2048
N_SEEDED = 384
AIMED_PER_ROW = 24
AIM_DRAWS = 6000
TIE = 1e-9
STALE_SLOT = (0.9, -0.7)
DROP_CAP = 0.02

OPTION_SETS = {
    "default": dict(),
    "zero_radius": dict(pMin=1.0, pMax=1.0),   # lo(Lgh) == hi(Lgh): the two rows of a pair coincide
    "straddle": dict(pMin=-0.5, pMax=1.5),     # lo(Lgh) < 0 < hi(Lgh)
    "tight_box": dict(lb=-0.3, ub=0.2),        # asymmetric and tight: u* sits on a bound
    "relax": dict(relaxLb=0.0, relaxCost=5.0),
}
PM_SETS = ("default", "zero_radius", "straddle")  # the sets that change the assembled rows


def options(lib, N, name="default", phase=PHASE):
    """The named option set for N half-planes on lib's C5 defaults; lib is oracle_lib or asif_amd.capi."""
    o = lib.default_options(MODEL, VARIANT)
    o.nHalfPlanes = N
    for k in range(N, 8):  # slots the filter must not read: half-planes that would change most answers if it did
        o.halfPlanes[2 * k], o.halfPlanes[2 * k + 1] = STALE_SLOT
    for k in range(N):
        th = 2 * np.pi * (k + phase) / N
        o.halfPlanes[2 * k] = np.cos(th) / np.pi
        o.halfPlanes[2 * k + 1] = np.sin(th) / np.pi
    for k, v in OPTION_SETS[name].items():
        if k in ("lb", "ub"):
            getattr(o, k)[0] = v
        else:
            setattr(o, k, v)
    return o


def _facet_frame(N, s, phase):
    th = 2 * np.pi * (s + phase) / N
    nrm = np.stack([np.cos(th), np.sin(th)], axis=1)
    tng = np.stack([-np.sin(th), np.cos(th)], axis=1)
    half = min(np.pi * np.tan(np.pi / N), 3.0) if N >= 3 else 3.0  # half a facet's length (N < 3: the set is unbounded)
    return th, nrm, tng, half


def _scattered(N, m, rng, phase):
    """m states on the facets' lines, moved off them to either side, uDes of both signs."""
    s = np.arange(m) % N
    _, nrm, tng, half = _facet_frame(N, s, phase)
    t = rng.uniform(-1.5, 1.5, m) * half
    near = rng.uniform(size=m) < 0.7
    dist = np.where(near, rng.uniform(0.01, 0.35, m) * np.where(rng.uniform(size=m) < 0.5, 1.0, -1.0),
                    rng.uniform(0.35, 1.2, m))  # > 0: inside
    x = (np.pi - dist)[:, None] * nrm + t[:, None] * tng
    u = rng.uniform(0.05, 1.5, m) * np.where((np.arange(m) // N) % 2 == 0, 1.0, -1.0)
    return x, u[:, None]


def _aimed(o, N, rng, phase):
    """(x, uDes, s, p): states aimed at an optimum with the reduced row (s, p) alone active.  With the row
    g u + h delta >= -Lfh active at multiplier lam > 0 the optimum is u* = uDes + lam g / 2, delta* = relaxLb +
    lam h / (2 relaxCost).  AIM_DRAWS states per row are drawn in a band inside the facet's line (reaching past the
    facet's ends); a state is kept where the u at which the row is tight at delta = relaxLb has p's sign and lies inside
    the input box, and uDes is put 0.02 ... 0.6 beyond the resulting u* on the side the row pushes back from.  Whether
    another row interferes is the oracle's to say (_candidates)."""
    s = np.repeat(np.arange(N), 2 * AIM_DRAWS)
    p = np.tile(np.repeat(np.arange(2), AIM_DRAWS), N)
    m = len(s)
    th, nrm, tng, half = _facet_frame(N, s, phase)
    a1 = np.sin(th) / np.pi
    ends = -a1[:, None] * np.array([o.pMin, o.pMax])[None, :]
    g = np.where(p == 0, ends.min(axis=1), ends.max(axis=1))
    t = rng.uniform(-1.7, 1.7, m) * half
    d = 0.004 + 2.5 * rng.uniform(size=m) ** 2
    x = (np.pi - d)[:, None] * nrm + t[:, None] * tng
    h = d / np.pi
    lfh = -(np.cos(th) * x[:, 1] + np.sin(th) * np.sin(x[:, 0])) / np.pi
    push = rng.uniform(0.02, 0.6, m)
    lam = 2.0 * push / np.abs(g)
    ustar = -(h * (o.relaxLb + lam * h / (2.0 * o.relaxCost)) + lfh) / g
    udes = ustar - lam * g / 2.0
    umax = np.where(p == 0, o.ub[0], -o.lb[0])
    sgn = np.where(p == 0, 1.0, -1.0)
    keep = (sgn * ustar > 0.05 * umax) & (sgn * ustar < 0.95 * umax)
    return x[keep], udes[keep, None], s[keep], p[keep]


def _candidates(oracle, N, n, rng, phase):
    """n candidate (x, uDes): N_SEEDED seeded C5 states; for every option set and every row, up to `per_row` aimed
    states on which the oracle finds that row binding; the rest scattered about the facets."""
    parts = [oracle.make_batch(5, N_SEEDED)]
    per_row = min(AIMED_PER_ROW, (n - N_SEEDED - n // 8) // (2 * N * len(OPTION_SETS)))
    for name in OPTION_SETS:
        o = options(oracle, N, name, phase)
        x, u, s, p = _aimed(o, N, rng, phase)
        # the oracle's word on a few times as many as are needed
        first = np.concatenate([np.where((s == a) & (p == b))[0][:4 * per_row] for a in range(N) for b in range(2)])
        x, u, s, p = x[first], u[first], s[first], p[first]
        if len(x) == 0:
            continue
        ua, rl, rc = oracle.filter_batch(MODEL, VARIANT, o, x, u, oracle.SOLVER_EXACT)
        hit = binding(o, reduced_qp(oracle, o, x, u), u, ua, rl, rc)[np.arange(len(x)), s, p]
        pick = np.concatenate([np.where(hit & (s == a) & (p == b))[0][:per_row] for a in range(N) for b in range(2)])
        parts.append((x[pick], u[pick]))
    m = n - sum(len(q[0]) for q in parts)
    parts.append(_scattered(N, m, rng, phase))
    return np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])


def reduced_qp(oracle, o, x, udes):
    """The 2-variable QP of every instance, AoS for oracle.qp_solve_batch: Hd, c, A [n, 2N*2] column-major, b, lb, ub."""
    N = o.nHalfPlanes
    d = oracle.dims(MODEL, VARIANT, o)
    n = len(x)
    Af, _, code, _ = oracle.assemble_batch(MODEL, VARIANT, o, x)
    assert np.all(code == 1)
    Af = Af.reshape(n, d.nv, d.nc)  # [instance, col, row]
    A = np.zeros((n, 2, 2 * N))
    b = np.zeros((n, 2 * N))
    for s in range(N):
        row, col = 3 * s, 2 + 4 * s
        A[:, 0, 2 * s] = Af[:, col, row]            # lo(Lgh)
        A[:, 0, 2 * s + 1] = -Af[:, col + 2, row]   # hi(Lgh)
        A[:, 1, 2 * s] = A[:, 1, 2 * s + 1] = Af[:, 1, row]  # h
        b[:, 2 * s] = b[:, 2 * s + 1] = -Af[:, col + 1, row]  # -lo(Lfh)
    Hd = np.tile([1.0, o.relaxCost], (n, 1))
    c = np.stack([-2.0 * udes[:, 0], np.full(n, -2.0 * o.relaxCost * o.relaxLb)], axis=1)
    lb = np.tile([o.lb[0], o.relaxLb], (n, 1))
    ub = np.tile([o.ub[0], o.inf], (n, 1))
    return Hd, c, A.reshape(n, -1), b, lb, ub


def slacks(o, qp, ua, rl):
    """Scaled slack of every reduced row at (ua, rl): [n, 2N], (a . z - b) / (1 + |a| . |z| + |b|)."""
    _, _, A, b, _, _ = qp
    n = len(b)
    A = A.reshape(n, 2, -1)
    z = np.stack([ua[:, 0], rl[:, 0]], axis=1)
    az = A[:, 0] * z[:, :1] + A[:, 1] * z[:, 1:]
    mag = 1.0 + np.abs(A[:, 0] * z[:, :1]) + np.abs(A[:, 1] * z[:, 1:]) + np.abs(b)
    return (az - b) / mag


def binding(o, qp, udes, ua, rl, rc):
    """bool [n, N, 2]: row (s, p) binds on the instance (see the module's docstring)."""
    N = o.nHalfPlanes
    ok = rc == 1
    with np.errstate(invalid="ignore"):
        tight = np.abs(slacks(o, qp, ua, rl)) <= TIE
        moved = (np.abs(ua[:, 0] - np.clip(udes[:, 0], o.lb[0], o.ub[0])) > TIE) | (rl[:, 0] > o.relaxLb + TIE)
        sign = np.stack([ua[:, 0] > 0, ua[:, 0] < 0], axis=1)
    return tight.reshape(-1, N, 2) & (ok & moved)[:, None, None] & sign[:, None, :]


def _well_posed(oracle, o, x, udes):
    qp = reduced_qp(oracle, o, x, udes)
    Hd, c, A, b, lb, ub = qp
    N = o.nHalfPlanes
    n = len(x)
    sol, st, _ = oracle.qp_solve_batch(2, 2 * N, Hd, c, A, b, lb, ub, solver=oracle.SOLVER_EXACT)
    ok = np.ones(n, bool)
    for sgn in (1.0, -1.0):
        bs = b + sgn * TIE * (1.0 + np.abs(b))
        ok &= (oracle.qp_solve_batch(2, 2 * N, Hd, c, A, bs, lb, ub, solver=oracle.SOLVER_EXACT)[1] == 1) == (st == 1)
    # constraints tight at the optimum, rows with the same coefficients once
    m = st == 1
    with np.errstate(invalid="ignore"):
        tight = np.abs(slacks(o, qp, sol[:, :1], sol[:, 1:])) <= TIE
        A3 = A.reshape(n, 2, 2 * N)
        dup = np.zeros_like(tight)
        dup[:, 1::2] = tight[:, 0::2] & (A3[:, 0, 1::2] == A3[:, 0, 0::2])  # hi row == lo row (zero radius)
        cnt = (tight & ~dup).sum(axis=1)
        cnt += (np.abs(sol[:, 0] - o.lb[0]) <= TIE).astype(int) + (np.abs(sol[:, 0] - o.ub[0]) <= TIE)
        cnt += np.abs(sol[:, 1] - o.relaxLb) <= TIE
    ok &= ~m | (cnt <= 2)
    return ok


_cache = {}


def family(oracle, N, ph=0, seed=5150):
    """dict(N; x [B,2], udes [B,1] AoS; xs [2,B], udes_s [1,B] SoA for the device; drawn, dropped: the candidates
    drawn and left out; sets: name -> dict(o: the oracle's options, ua [B,1], rl [B,1], rc [B]: the oracle's exact
    filter on the batch, relax NaN where rc != 1))."""
    if (N, ph) in _cache:
        return _cache[N, ph]
    phase = phases(N)[ph]
    rng = np.random.default_rng(seed + 16 * ph + N)
    drawn = B + B // 64
    x, udes = _candidates(oracle, N, drawn, rng, phase)
    ok = np.ones(drawn, bool)
    for name in OPTION_SETS:
        ok &= _well_posed(oracle, options(oracle, N, name, phase), x, udes)
    dropped = int((~ok).sum())
    assert dropped <= DROP_CAP * drawn, (N, dropped, drawn)
    keep = np.where(ok)[0][:B]
    assert len(keep) == B
    keep = keep[rng.permutation(B)]  # every span of 64 mixes seeded and facet states
    x, udes = np.ascontiguousarray(x[keep]), np.ascontiguousarray(udes[keep])
    sets = {}
    for name in OPTION_SETS:
        o = options(oracle, N, name, phase)
        ua, rl, rc = oracle.filter_batch(MODEL, VARIANT, o, x, udes, oracle.SOLVER_EXACT)
        sets[name] = dict(o=o, ua=ua, rl=rl, rc=rc)
    fam = dict(N=N, ph=ph, phase=phase, x=x, udes=udes, xs=np.ascontiguousarray(x.T), udes_s=np.ascontiguousarray(udes.T), drawn=drawn,
               dropped=dropped, sets=sets)
    for v in [x, udes] + [a for s in sets.values() for a in (s["ua"], s["rl"], s["rc"])]:
        v.setflags(write=False)
    _cache[N, ph] = fam
    return fam


def binding_counts(oracle, fam, name):
    """int [N, 2]: instances on which row (s, lo / hi) binds under the named option set."""
    s = fam["sets"][name]
    qp = reduced_qp(oracle, s["o"], fam["x"], fam["udes"])
    return binding(s["o"], qp, fam["udes"], s["ua"], s["rl"], s["rc"]).sum(axis=0)
