"""Independent check of the one assembly with no reference-derived pin at all: the time-to-safety row and the
orthogonality row of ASIFimplicitTB (src/asif_implicit_tb.cpp:588-641) as the oracle restates them.

Both rows are gradients THROUGH THE HITTING MAP x0 -> phi_tau(x0)(x0) of the backup trajectory:
    d tau / d x0 = -(grad h_B . Q) / (grad h_B . fCL)            (implicit function theorem at h_B = 0)
so the test recomputes the hitting time and the angle at the hit from scratch -- its own closed loop of
examples/InvertedPendulum_ImplicitTB.cpp (velocity-tracking controller, bevelled saturation, pendulum dynamics)
integrated with RK4 (fourth order at the same step: far below the O(dt) of the oracle's Euler), the crossing located by bisection on a dense output -- and differentiates
them by central differences along g.  The oracle's rows use forward Euler at dt = 1e-3 and evaluate at the first
SAMPLE inside the backup set, so agreement is expected to O(dt): rtol 3e-2.  A wrong sign, a missing 1/cos factor or a
transposed sensitivity would be off by O(1).

The orthogonality row is NOT the true derivative in the reference: it pushes the state through
J = Q - fCL (grad h_B Q) without the 1 / (grad h_B . fCL) of the hitting map and books the derivative of |fCL| under
|grad h_B| (src/asif_implicit_tb.cpp:601-641; SURVEY App. B "preserve").  For a half-space backup set (Hessian 0,
|grad h_B| = 1) that formula collapses to
    row = (1 - grad h_B . fCL) / |fCL|  *  grad h_B' DfCL J ,
which the second test evaluates with a sensitivity Q obtained by differencing this file's own flow at the hit time."""
import numpy as np
import pytest

LB, UB, R_SAT = -1.5, 1.5, 0.1


def _sat(u, LB=LB, UB=UB):
    rng, mid = UB - LB, 0.5 * (UB + LB)
    uc = 2.0 * (u - mid) / rng
    bev = R_SAT * np.tan(np.pi / 8)
    start, stop, yc = 1 - np.cos(np.pi / 4) * bev, 1 + bev, 1 - R_SAT
    if abs(uc) <= start:
        return u
    if abs(uc) >= stop:
        return UB if uc > 0 else LB
    s = np.sqrt(R_SAT ** 2 - (abs(uc) - stop) ** 2)
    return np.sign(uc) * 0.5 * (s + yc) * rng + mid


def _fcl(x):
    u = 10.0 * (np.pi / 10.0 - x[1])
    return np.array([x[1], np.sin(x[0]) + _sat(u)])


def _hb(x):
    return x[0] - np.pi / 2 + 0.1


def _hit(x0, dt=1e-3, tmax=12.0):
    """(tau, state at the crossing) of the continuous backup flow."""
    x, t = np.array(x0, dtype=float), 0.0
    assert _hb(x) < 0
    while t < tmax:
        k1 = _fcl(x); k2 = _fcl(x + 0.5 * dt * k1); k3 = _fcl(x + 0.5 * dt * k2); k4 = _fcl(x + dt * k3)
        xn = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        if _hb(xn) >= 0:
            lo, hi = 0.0, dt  # bisection on a cubic-Hermite-free substitute: re-integrate the fraction of the step
            for _ in range(50):
                m = 0.5 * (lo + hi)
                k1 = _fcl(x); k2 = _fcl(x + 0.5 * m * k1); k3 = _fcl(x + 0.5 * m * k2); k4 = _fcl(x + m * k3)
                xm = x + m / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
                if _hb(xm) >= 0:
                    hi = m
                else:
                    lo = m
            return t + hi, xm
        x, t = xn, t + dt
    raise AssertionError("backup set not reached")


def _flow(x0, T, dt=1e-3):
    x = np.array(x0, dtype=float)
    n = int(round(T / dt))
    for _ in range(n):
        k1 = _fcl(x); k2 = _fcl(x + 0.5 * dt * k1); k3 = _fcl(x + 0.5 * dt * k2); k4 = _fcl(x + dt * k3)
        x = x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def _ortho(xh):
    f = _fcl(xh)  # grad h_B = (1, 0)
    return f[0] / np.hypot(f[0], f[1])


def test_tts_and_ortho_rows_are_derivatives_through_the_hitting_map(oracle):
    model, variant = oracle.MODEL_IP_TB, oracle.VAR_TB
    o = oracle.default_options(model, variant)
    d = oracle.dims(model, variant, o)
    assert (d.nv, d.nc) == (2, 18)
    x, _ = oracle.make_batch(8, 96)
    A, b, code, diag = oracle.assemble_batch(model, variant, o, x)
    idx = np.where(code == 1)[0]
    assert len(idx) >= 12
    g = np.array([0.0, 1.0])
    f_at = lambda xx: np.array([xx[1], np.sin(xx[0])])
    eps = 1e-5
    checked = 0
    for k in idx[:12]:
        Am = A[k].reshape(2, 18).T
        tau0, xh0 = _hit(x[k])
        # the oracle's own numbers first: hitting time (sample grid) and cosine at the hit
        assert abs(diag[k, 0] - tau0) <= 2e-3 + 1e-3 * tau0, (diag[k, 0], tau0)  # Euler at dt 1e-3 + the sample grid
        assert abs(diag[k, 1] - _ortho(xh0)) <= 5e-3
        taup, xhp = _hit(x[k] + eps * g)
        taum, xhm = _hit(x[k] - eps * g)
        dtau_g = (taup - taum) / (2 * eps)
        dort_g = (_ortho(xhp) - _ortho(xhm)) / (2 * eps)
        # TTS row: h = T - tau  ->  Lgh = -d tau . g ;  b = -Lfh - relaxTTS h with Lfh = -d tau . f
        np.testing.assert_allclose(Am[16, 0], -dtau_g, rtol=3e-2, atol=2e-4)
        del dort_g  # the reference's orthogonality row is not this derivative: see the module docstring and the next test
        # the same two gradients contracted with f(x0) sit in b
        tf_p, xf_p = _hit(x[k] + eps * f_at(x[k]))
        tf_m, xf_m = _hit(x[k] - eps * f_at(x[k]))
        dtau_f = (tf_p - tf_m) / (2 * eps)
        hreach = o.backTrajHorizon - diag[k, 0]
        np.testing.assert_allclose(b[k, 16], dtau_f - o.relaxTTS * hreach, rtol=3e-2, atol=5e-3)
        checked += 1
    assert checked >= 10


def test_ortho_row_is_the_reference_formula(oracle):
    model, variant = oracle.MODEL_IP_TB, oracle.VAR_TB
    o = oracle.default_options(model, variant)
    x, _ = oracle.make_batch(8, 96)
    A, b, code, diag = oracle.assemble_batch(model, variant, o, x)
    idx = np.where(code == 1)[0]
    g = np.array([0.0, 1.0])
    eps = 1e-6
    checked = 0
    for k in idx[:24]:
        th = diag[k, 0]  # time of the first sample inside the backup set
        xh = _flow(x[k], th)
        u = 10.0 * (np.pi / 10.0 - xh[1])
        uc = 2.0 * u / (UB - LB)
        bev = R_SAT * np.tan(np.pi / 8)
        if 1 - np.cos(np.pi / 4) * bev < abs(uc) < 1 + bev:
            continue  # on a bevel of the saturation the reference's DuSat convention enters: keep to the plain regions
        dsat = 1.0 if abs(uc) < 1 else 0.0
        DfCL = np.array([[0.0, 1.0], [np.cos(xh[0]), -10.0 * dsat]])
        Q = np.stack([(_flow(x[k] + eps * e, th) - _flow(x[k] - eps * e, th)) / (2 * eps) for e in np.eye(2)], axis=1)
        f = _fcl(xh)
        gh = np.array([1.0, 0.0])
        J = Q - np.outer(f, gh @ Q)
        row = (1.0 - gh @ f) / np.linalg.norm(f) * (gh @ DfCL @ J)
        Am = A[k].reshape(2, 18).T
        np.testing.assert_allclose(Am[17, 0], row @ g, rtol=5e-2, atol=2e-4)
        checked += 1
    assert checked >= 8


# ---- the segway on states that reach the backup set late (tests/synth_states.py).  The check through the CONTINUOUS
# hitting map above does not carry over: the segway's backup set is a small ellipsoid (0.157 rad/s wide in the pitch
# rate) that the closed loop crosses in a few Euler steps, so the sample at which forward Euler lands inside it is not
# within O(dt) of where the continuous flow crosses (measured with RK4 + bisection: the two derivatives differ by
# 10 % to 30 x).  Nor are the rows derivatives of the map the class integrates: the example zeroes the friction term
# in f and ships the Jacobian generated WITH it (examples/segway_implicit_tb.cpp:78 against :113-212), so the
# sensitivity is Q_{i+1} = Q_i + dt DfCL~(x_i) Q_i along the friction-free trajectory x_i, DfCL~ the Jacobian of the
# closed loop with friction (measured: differencing the integrated flow itself is off by O(1) in some rows).  That
# recursion is what is rebuilt here, with DfCL~(x_i) w taken by central differences of the flow alone (the oracle's
# fCl - f + fDiff export): the transcribed Jacobian, the saturation's slope, the recursion over up to 315 steps and the
# row formulas at the critical samples and at the hit are checked against something that contains none of them.

def _euler_path(fcl, x0, dt, n):
    """[n, B, nx]: the samples of forward Euler from the rows of x0, with the oracle's own two roundings per step."""
    out = np.empty((n,) + x0.shape)
    out[0] = x0
    for i in range(1, n):
        out[i] = fcl(out[i - 1]) * dt + out[i - 1]
    return out


def _central(fun, x, v, eps):
    """d fun(x + s v) / ds at 0 by central differences, v scaled to unit length per row for the step."""
    s = np.linalg.norm(v, axis=-1, keepdims=True)
    s = np.where(s > 0, s, 1.0)
    return (fun(x + eps * v / s) - fun(x - eps * v / s)) / (2 * eps) * s


@pytest.mark.parametrize("name", ["fine_step", "default"])
def test_segway_rows_on_late_hits_against_a_differenced_flow(oracle, name):
    import synth_states as S
    fam = S.late_hit_family(oracle, name)
    o, npBT, dt = fam["o"], fam["npBT"], fam["o"].backTrajDt
    ev = lambda X: oracle.model_eval(S.MODEL, S.VARIANT, o, X)
    fcl = lambda X: ev(X)["fCl"]

    def fcl_diff(X):  # the closed loop whose Jacobian the class propagates
        e = ev(X)
        return e["fCl"] - e["f"] + e["fDiff"]
    hit = fam["diag"][:, 2].astype(int)
    m = fam["code"] == 1
    # a sample over the whole trajectory: past the first two blocks, some in the last block and on the last sample
    late = np.where(m & (hit >= 2 * S.BLOCK) & (hit < npBT - S.BLOCK))[0]
    idx = np.concatenate([late[:: max(1, len(late) // 16)][:16], np.where(m & (hit >= npBT - S.BLOCK))[0][:6],
                          np.where(m & (hit == npBT - 1))[0][:2]])
    x, k, crit = fam["x"][idx], hit[idx], fam["crit"][idx]
    n = len(idx)
    assert n >= 20 and np.all(crit >= 0)
    e0 = ev(x)
    rows = np.arange(n)
    A = fam["A"][idx].reshape(n, 2, 18)
    b = fam["b"][idx]
    X = _euler_path(fcl, x, dt, npBT)
    xk, xc = X[k, rows], X[crit.T, rows]  # hit sample [n, nx]; critical samples [4, n, nx]
    ek = ev(xk)
    fk, Dh = ek["fCl"], ek["DhBS"]
    cos = (Dh * fk).sum(axis=1)
    den1, den2 = np.linalg.norm(Dh, axis=1), np.linalg.norm(fk, axis=1)
    den = den1 * den2
    np.testing.assert_allclose(fam["diag"][idx, 1], cos / den, rtol=1e-12)  # BTorthoBS_ itself
    np.testing.assert_allclose(fam["diag"][idx, 0], k * dt, rtol=1e-12)     # TTS_ (accumulated sample times)
    np.testing.assert_allclose(A[:, 1, :16], (S.XB ** 2 - xc ** 2).transpose(1, 0, 2).reshape(n, 16), rtol=1e-12)
    assert np.all(A[:, 1, 16:] == 0.0)

    def rows_from(v, eps):
        P = np.empty((npBT, n, 4))
        P[0] = v
        for i in range(1, npBT):
            P[i] = P[i - 1] + dt * _central(fcl_diff, X[i - 1], P[i - 1], eps)
        out = np.zeros((n, 18))
        for j in range(4):  # safety rows: h_i = xBound_i^2 - x_i^2 at the four critical samples
            out[:, 4 * j:4 * j + 4] = -2.0 * xc[j] * P[crit[:, j], rows]
        Qv = P[k, rows]
        DhQv = (Dh * Qv).sum(axis=1)
        out[:, 16] = DhQv / cos  # time-to-safety row
        # orthogonality row as the reference books it (module docstring), its two Jacobians differenced too
        Jv = Qv - fk * DhQv[:, None]
        t2 = _central(fcl_diff, xk, Jv, eps)
        t1 = _central(lambda Y: ev(Y)["DhBS"], xk, Jv, eps)
        Dden1, Dden2 = (Dh * t2).sum(axis=1), (t1 * fk).sum(axis=1)
        Dden = den2 * Dden1 / den1 + den1 * Dden2 / den2
        out[:, 17] = ((Dden1 + Dden2) * den - cos * Dden) / (den * den)
        return out

    for v, got, sign, in_b in ((e0["g"], A[:, 0, :], 1.0, False), (e0["f"], b, -1.0, True)):
        want = sign * rows_from(v, 1e-6)
        err = np.abs(sign * rows_from(v, 2e-6) - want)
        if in_b:  # b carries the relaxation of the two extra rows
            want[:, 16] -= o.relaxTTS * (o.backTrajHorizon - k * dt)
            want[:, 17] -= o.relaxMinOrtho * (cos / den - o.backTrajMinOrtho)
        # bound: the difference quotients' own error, read off the same computation at twice the step (truncation is a
        # third of that for a smooth map; the saturation's bevels and tanh(1000 x1) are not smooth at that scale, hence
        # the whole of it), plus their rounding: 1e-16 |fCl| / eps = 1e-10 per step and unit, 300 steps, and a factor 30
        # for the cancellation in the rows -- 1e-6 of the instance's largest row entry
        tol = err + 1e-6 * np.abs(want).max(axis=1, keepdims=True)
        gap = np.abs(got - want)
        print(f"\n{name} {'b' if in_b else 'A'}: worst |row - rebuilt row| = {(gap / tol).max():.3g} of its bound, "
              f"{(gap / np.abs(want).max(axis=1, keepdims=True)).max():.3g} of the instance's largest entry")
        assert np.all(gap <= tol), (np.argwhere(gap > tol)[:5], (gap / tol).max())


# ---- the double integrator of examples/DoubleIntegrator_implicit_tb.cpp: a CURVED backup set (disc of radius 0.01),
# so the hit moves along the boundary with x0 and the Hessian term of the rows is live

def _di_fcl(x):
    return np.array([x[1], _sat(-10.0 * x[0] - 20.0 * x[1], -1.0, 1.0)])


def _di_hit(x0, dt=1e-3, tmax=2.2):
    hb = lambda xx: 1e-4 - xx @ xx
    rk = lambda xx, h: (lambda k1: (lambda k2: (lambda k3: xx + h / 6 * (k1 + 2 * k2 + 2 * k3 + _di_fcl(xx + h * k3)))(
        _di_fcl(xx + 0.5 * h * k2)))(_di_fcl(xx + 0.5 * h * k1)))(_di_fcl(xx))
    x, t = np.array(x0, dtype=float), 0.0
    assert hb(x) < 0
    while t < tmax:
        xn = rk(x, dt)
        if hb(xn) >= 0:
            lo, hi = 0.0, dt
            for _ in range(50):
                m = 0.5 * (lo + hi)
                if hb(rk(x, m)) >= 0:
                    hi = m
                else:
                    lo = m
            return t + hi
        x, t = xn, t + dt
    raise AssertionError("backup set not reached")


def test_tts_row_with_a_curved_backup_set(oracle):
    model, variant = oracle.CONFIGS[12]
    o = oracle.default_options(model, variant)
    d = oracle.dims(model, variant, o)
    assert (d.nv, d.nc, d.npBT) == (2, 18, 2101)
    x, _ = oracle.make_batch(12, 160)
    A, b, code, diag = oracle.assemble_batch(model, variant, o, x)
    idx = [k for k in np.where(code == 1)[0] if 0.2 < diag[k, 0] < 1.9]  # away from the horizon's end and from t = 0
    assert len(idx) >= 12
    g = np.array([0.0, 1.0])
    eps = 1e-6
    checked = 0
    for k in idx[:16]:
        Am = A[k].reshape(2, 18).T
        tau0 = _di_hit(x[k])
        assert abs(diag[k, 0] - tau0) <= 2e-3 + 2e-3 * tau0, (diag[k, 0], tau0)
        dtau_g = (_di_hit(x[k] + eps * g) - _di_hit(x[k] - eps * g)) / (2 * eps)
        np.testing.assert_allclose(Am[16, 0], -dtau_g, rtol=3e-2, atol=2e-4)
        f0 = np.array([x[k][1], 0.0])
        dtau_f = (_di_hit(x[k] + eps * f0) - _di_hit(x[k] - eps * f0)) / (2 * eps)
        hreach = o.backTrajHorizon - diag[k, 0]
        np.testing.assert_allclose(b[k, 16], dtau_f - o.relaxTTS * hreach, rtol=3e-2, atol=5e-3)
        checked += 1
    assert checked >= 12
