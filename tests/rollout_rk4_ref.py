"""Reference for the fused rollout under an affine policy with the plant stepped by RK4 under a held input, and its exact
discrete adjoint (asif_hip_rollout_plant_batch / asif_hip_rollout_plant_vjp_batch with ASIF_HIP_PLANT_RK4), in numpy.

TEST INFRASTRUCTURE, not a test.  The model, the filter step, the policy and the filter's adjoint are those of the module
handed in -- tests/rollout_params_ref.py (double integrator) or tests/cart_pendulum_ref.py (cart-driven pendulum); nothing
of them is copied.  Both are wrapped step by step: their forward() and adjoint() called on ONE step with dt = 0 are the
filter call alone (the Euler terms they add are dt times something), and the plant's part is restated here.

The step, u = u_t held, F(X, u) = f(X) + g(X) u, every product and sum rounded on its own, in this order
(asif_amd/csrc/plant_step.hpp):
    F_k(X) = (0 + f_k) + u g_k
    k1 = F(x);  X2 = x + (0.5 dt) k1;  k2 = F(X2);  X3 = x + (0.5 dt) k2;  k3 = F(X3);  X4 = x + dt k3;  k4 = F(X4)
    x+ = x + (dt / 6) (((k1 + 2 k2) + 2 k3) + k4)
Its adjoint, lambda = dL/dx+, J_i = Df(X_i) + u Dg(X_i):
    kb4 = dt/6 lambda;              Xb4 = J4' kb4
    kb3 = dt/3 lambda + dt   Xb4;   Xb3 = J3' kb3
    kb2 = dt/3 lambda + dt/2 Xb3;   Xb2 = J2' kb2
    kb1 = dt/6 lambda + dt/2 Xb2;   Xb1 = J1' kb1
    mu += gulog[t] + sum_i g(X_i)' kb_i;    lambda' = lambda + Xb1 + Xb2 + Xb3 + Xb4 + gxlog[t]
then the filter's adjoint at x_t with gbar = mu, unchanged.  The filter is evaluated at the sample instants only.
"""
import numpy as np

NX, NU = 2, 1


def dynamics(mod, X):
    """f [B,2], g [B,2], Df [B,2,2], Dg [B,2,2] (d . _k / d x_m at [k,m]) of mod's model at X [2,B]."""
    out = mod.model(X)
    f, g, Df = out[3], out[4], out[5]
    Dg = out[6] if len(out) > 6 else np.zeros_like(Df)
    return f, g, Df, Dg


def closed_loop(f, g, u):
    """F(X, u) [2,B] in the documented order."""
    return np.stack([(0.0 + f[:, m]) + u * g[:, m] for m in range(NX)])


def stages(mod, x, u, dt):
    """The four stage states [4][2,B] and slopes [4][2,B] from (x, u)."""
    hdt = 0.5 * dt
    X, k = [x], []
    for c in (hdt, hdt, dt):
        f, g, _, _ = dynamics(mod, X[-1])
        k.append(closed_loop(f, g, u))
        X.append(x + c * k[-1])
    f, g, _, _ = dynamics(mod, X[-1])
    k.append(closed_loop(f, g, u))
    return X, k


def rk4_step(mod, x, u, dt):
    """x [2,B], u [B] -> x+ [2,B]."""
    _, k = stages(mod, x, u, dt)
    return x + (dt / 6.0) * (((k[0] + 2.0 * k[1]) + 2.0 * k[2]) + k[3])


def euler_step(mod, x, u, dt):
    """The kernels' Euler step in their order: x + dt ((0 + f) + u g)."""
    f, g, _, _ = dynamics(mod, x)
    return x + dt * closed_loop(f, g, u)


def rk4_step_adjoint(mod, x, u, dt, lam, mu):
    """lam [B,2] = dL/dx+, mu [B] -> (lam + sum_i Xb_i, mu + sum_i g_i' kb_i, the largest |Xb_i| or |kb_i| met [B])."""
    X, _ = stages(mod, x, u, dt)
    D = [dynamics(mod, Xi) for Xi in X]
    J = [Df + u[:, None, None] * Dg for _, _, Df, Dg in D]
    back = lambda i, kb: np.einsum("bkm,bk->bm", J[i], kb)
    kb4 = (dt / 6.0) * lam
    Xb4 = back(3, kb4)
    kb3 = (dt / 3.0) * lam + dt * Xb4
    Xb3 = back(2, kb3)
    kb2 = (dt / 3.0) * lam + (0.5 * dt) * Xb3
    Xb2 = back(1, kb2)
    kb1 = (dt / 6.0) * lam + (0.5 * dt) * Xb2
    Xb1 = back(0, kb1)
    gu = sum(np.einsum("bk,bk->b", D[i][1], kb) for i, kb in enumerate((kb1, kb2, kb3, kb4)))
    big = np.max([np.abs(a).max(axis=1) for a in (kb1, kb2, kb3, kb4, Xb1, Xb2, Xb3, Xb4)], axis=0)
    return lam + (((Xb4 + Xb3) + Xb2) + Xb1), mu + gu, big


def forward(mod, x0, k, K, v, uact_prev, T, dt, opt, alpha=None, lb=None, ub=None, plant="rk4"):
    """mod.forward's arguments and keys, with the plant stepped by RK4 (plant="euler": mod's own step, through the same
    wrapping)."""
    B = x0.shape[1]
    x, u = x0.copy(), uact_prev.copy()
    xlog, ulog, udl = np.zeros((T, NX, B)), np.zeros((T, NU, B)), np.zeros((T, B))
    rclog, wid = np.zeros((T, B), dtype=np.int32), np.zeros((T, B), dtype=int)
    step = rk4_step if plant == "rk4" else euler_step
    for t in range(T):
        with np.errstate(invalid="ignore"):  # dt = 0: the filter call alone; 0 * inf of a wild state is not looked at
            s = mod.forward(x, k, K, None if v is None else v[t:t + 1], u, 1, 0.0, opt, alpha, lb, ub)
        xlog[t], ulog[t], rclog[t], wid[t], udl[t] = x, s["ulog"][0], s["rclog"][0], s["wid"][0], s["udes"][0]
        u = s["uactT"]
        with np.errstate(invalid="ignore", over="ignore"):
            x = step(mod, x, u[0], dt)
    return dict(xT=x, uactT=u.copy(), xlog=xlog, ulog=ulog, rclog=rclog, wid=wid, udes=udl)


def adjoint(mod, xlog, ulog, rclog, k, K, v, dt, opt, gxT, guactT=None, gxlog=None, gulog=None, alpha=None, lb=None,
            ub=None, plant="rk4"):
    """mod.adjoint's arguments and keys on RK4 logs.  plant="euler" is the SWITCH of the tests: the Euler adjoint of the
    plant on the same logs -- what a sweep that ignored the integrator would compute.  S [B] also covers the stage
    adjoints kb_i, Xb_i."""
    T, _, B = xlog.shape if xlog is not None and len(xlog) else (0, NX, gxT.shape[1])
    lam = gxT.copy()                                         # [2,B]
    mu = guactT.copy() if guactT is not None else np.zeros((1, B))
    gk = np.zeros((1, B))
    gK = np.zeros((NX, B)) if K is not None else None
    gv = np.zeros((T, NU, B)) if v is not None else None
    ga = np.zeros(B) if alpha is not None else None
    gl = np.zeros((1, B)) if lb is not None else None
    gu = np.zeros((1, B)) if ub is not None else None
    nrow = nlb = nub = 0
    S = np.maximum(np.abs(lam).max(axis=0), np.abs(mu[0]))
    amin = np.ones(B)
    for t in range(T - 1, -1, -1):
        one = slice(t, t + 1)
        gxl = gxlog[one] if gxlog is not None else None
        gul = gulog[one] if gulog is not None else None
        if plant == "rk4":
            with np.errstate(invalid="ignore", over="ignore"):
                l2, m2, big = rk4_step_adjoint(mod, xlog[t], ulog[t, 0], dt, lam.T, mu[0])
            lam = l2.T + (gxl[0] if gxl is not None else 0.0)
            mu = (m2 + (gul[0, 0] if gul is not None else 0.0))[None, :]
            S = np.maximum(S, np.where(np.isfinite(big), big, 0.0))
            sdt, gxl, gul = 0.0, None, None                  # the filter's adjoint alone
        else:
            sdt = dt
        with np.errstate(invalid="ignore"):
            a = mod.adjoint(xlog[one], ulog[one], rclog[one], k, K, None if v is None else v[one], sdt, opt, lam, mu, gxl,
                            gul, alpha, lb, ub)
        lam, mu = a["gx0"], a["guact0"]
        gk = gk + a["gk"]
        if gK is not None:
            gK = gK + a["gK"]
        if gv is not None:
            gv[t] = a["gv"][0]
        if ga is not None:
            ga = ga + a["galpha"]
        if gl is not None:
            gl = gl + a["glb"]
        if gu is not None:
            gu = gu + a["gub"]
        nrow, nlb, nub = nrow + a["nrow"], nlb + a["nlb"], nub + a["nub"]
        S, amin = np.maximum(S, a["S"]), np.minimum(amin, a["amin"])
    return dict(gx0=lam, gk=gk, gK=gK, gv=gv, guact0=mu, galpha=ga, glb=gl, gub=gu, nrow=nrow, nlb=nlb, nub=nub, S=S,
                amin=amin)


def census(fw):
    """cart_pendulum_ref.census for either model: failed / row / bound / free steps."""
    wid = fw["wid"]
    return dict(failed=int((wid == -2).sum()), row=int(((wid >= 0) & (wid < 4)).sum()), bound=int((wid >= 4).sum()),
                free=int((wid == -1).sum()))
