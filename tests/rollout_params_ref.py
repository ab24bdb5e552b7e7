"""Reference for the fused explicit rollout under an affine policy with the barrier gain and the input box per instance,
and its adjoint (asif_hip_rollout_params_batch / asif_hip_rollout_params_vjp_batch on the double integrator), in numpy.

TEST INFRASTRUCTURE, not a test.  The model and the plant step are those of tests/rollout_vjp_ref.py, the policy that of
tests/rollout_policy_ref.py; the one-variable projection is restated here with alpha [B], lb [B], ub [B] in the place of
the option block's three scalars.

Forward, t = 0 ... T-1, u_{-1} = uact_prev:
    uDes_t = k + K x_t + v_t
    (ok_t, u*_t) = the projection of uDes_t onto  { Lgh_r u >= -Lfh_r - alpha_i h_r,  lb_i <= u <= ub_i }
    u_t = ok_t ? u*_t : u_{t-1};   x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
A gain HANDED IN that is not a positive finite number fails every step of its instance; so do lb_i > ub_i and NaN data.
Adjoint, t = T-1 ... 0: the sweep of rollout_policy_ref.adjoint with alpha_i where it reads relaxLb, and on a solved step
that ends on W with w = mu / normal:
    W = safety row r:  galpha += -h_r w;    W = lower bound:  glb += w (= mu);    W = upper bound:  gub += -w (= mu)
"""
import numpy as np

from rollout_policy_ref import policy
from rollout_vjp_ref import ACTIVE_TOL, NP, NU, NX, model, options, plant_step  # noqa: F401  (re-exported)


def lane_params(opt, B, alpha=None, lb=None, ub=None):
    """alpha [B], lb [B], ub [B] (lb / ub handed in as [1,B]) and gain_ok [B]: the handle's value where None."""
    full = lambda v: np.full(B, float(v))
    al = full(opt["relaxLb"]) if alpha is None else np.asarray(alpha, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.ones(B, dtype=bool) if alpha is None else (al > 0.0) & (al < np.inf)
    return (al, full(opt["lb"]) if lb is None else np.asarray(lb[0], dtype=np.float64),
            full(opt["ub"]) if ub is None else np.asarray(ub[0], dtype=np.float64), ok)


def filter_step(x, udes, keep, al, lb, ub, gain_ok):
    """rollout_vjp_ref.filter_step with per-instance alpha, lb, ub [B]; same keys."""
    h, Dh, D2h, f, g, Df = model(x)
    B = udes.shape[0]
    Lfh = np.einsum("brk,bk->br", Dh, f)
    Lgh = np.einsum("brk,bk->br", Dh, g)
    a = Lgh.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b = -Lfh - h * al[:, None]
        if keep < NP:  # the rows of the `keep` smallest h; ties: lower index first
            pos = np.argsort(np.argsort(h, axis=1, kind="stable"), axis=1, kind="stable")
            drop = pos >= keep
            a[drop], b[drop] = 0.0, -1e20
        q = b / np.where(a != 0.0, a, 1.0)
        lo = np.fmax(lb, np.where(a > 0.0, q, -np.inf).max(axis=1))
        hi = np.fmin(ub, np.where(a < 0.0, q, np.inf).min(axis=1))
        u = np.fmin(np.fmax(udes, lo), hi)
        t = a * u[:, None]
        bad = ((b - t) > ACTIVE_TOL * (1.0 + np.abs(b) + np.abs(t))).any(axis=1)
        bad |= (lb - u > ACTIVE_TOL * (1.0 + np.abs(u) + np.abs(lb))) | (u - ub > ACTIVE_TOL * (1.0 + np.abs(u) + np.abs(ub)))
        bad |= ~(np.isfinite(al) & np.isfinite(lb) & np.isfinite(ub) & np.isfinite(udes)) | ~gain_ok
        up, down = u > udes, u < udes
        wid = np.full(B, -1)
        nrm = np.zeros(B)
        for r in range(NP - 1, -1, -1):  # lowest row first
            hit = (q[:, r] == u) & ((up & (a[:, r] > 0.0)) | (down & (a[:, r] < 0.0)))
            wid = np.where(hit, r, wid)
            nrm = np.where(hit, a[:, r], nrm)
        onlb, onub = (wid < 0) & up & (u == lb), (wid < 0) & down & (u == ub)
        wid = np.where(onlb, 4, np.where(onub, 5, wid))
        nrm = np.where(onlb, 1.0, np.where(onub, -1.0, nrm))
        uc = np.fmin(np.fmax(u, lb), ub)
    return dict(ok=~bad, u=uc, wid=wid, nrm=nrm, h=h, Dh=Dh, D2h=D2h, f=f, g=g, Df=Df, Lgh=Lgh)


def forward(x0, k, K, v, uact_prev, T, dt, opt, alpha=None, lb=None, ub=None):
    """rollout_policy_ref.forward with alpha [B], lb [1,B], ub [1,B], each or None (the handle's value); same keys."""
    B = x0.shape[1]
    par = lane_params(opt, B, alpha, lb, ub)
    x, u = x0.copy(), uact_prev[0].copy()
    xlog, ulog, udl = np.zeros((T, NX, B)), np.zeros((T, NU, B)), np.zeros((T, B))
    rclog, wid = np.zeros((T, B), dtype=np.int32), np.zeros((T, B), dtype=int)
    for t in range(T):
        xlog[t] = x
        udl[t] = policy(k, K, None if v is None else v[t], x)
        s = filter_step(x, udl[t], opt["keep"], *par)
        u = np.where(s["ok"], s["u"], u)
        ulog[t, 0] = u
        rclog[t] = np.where(s["ok"], 1, -1)
        wid[t] = np.where(s["ok"], s["wid"], -2)
        x = plant_step(x, u, dt)
    return dict(xT=x, uactT=u[None, :].copy(), xlog=xlog, ulog=ulog, rclog=rclog, wid=wid, udes=udl)


def adjoint(xlog, ulog, rclog, k, K, v, dt, opt, gxT, guactT=None, gxlog=None, gulog=None, alpha=None, lb=None, ub=None):
    """The sweep on given logs.  rollout_policy_ref.adjoint's keys, and galpha [B], glb [1,B], gub [1,B] (each None where
    the parameter is None), nrow / nlb / nub (steps with a nonzero contribution to each); S [B] also covers the largest
    |h_r w_r| met."""
    T, _, B = xlog.shape if xlog is not None and len(xlog) else (0, NX, gxT.shape[1])
    par = lane_params(opt, B, alpha, lb, ub)
    al = par[0]
    lam = gxT.T.copy()                                       # [B,2]
    mu = guactT[0].copy() if guactT is not None else np.zeros(B)
    gk = np.zeros(B)
    gK = np.zeros((NX, B)) if K is not None else None
    gv = np.zeros((T, NU, B)) if v is not None else None
    ga, gl, gu = np.zeros(B), np.zeros(B), np.zeros(B)
    nrow = nlb = nub = 0
    S = np.maximum(np.abs(lam).max(axis=1), np.abs(mu))
    amin = np.ones(B)
    idx = np.arange(B)
    for t in range(T - 1, -1, -1):
        x = xlog[t]
        s = filter_step(x, policy(k, K, None if v is None else v[t], x), opt["keep"], *par)
        Dh, D2h, f, g, Df = s["Dh"], s["D2h"], s["f"], s["g"], s["Df"]
        mu = mu + (gulog[t, 0] if gulog is not None else 0.0) + dt * np.einsum("bk,bk->b", g, lam)
        lamn = lam + dt * (lam @ Df)                         # (Df' lambda)_m = sum_k Df[k,m] lambda_k;  Dg = 0
        if gxlog is not None:
            lamn = lamn + gxlog[t].T
        S = np.maximum(S, np.maximum(np.abs(lamn).max(axis=1), np.abs(mu)))
        solved = rclog[t] == 1
        free = solved & (s["wid"] < 0)
        onrow = solved & (s["wid"] >= 0) & (s["wid"] < NP)
        onlb, onub = solved & (s["wid"] == 4), solved & (s["wid"] == 5)
        d = np.where(free, mu, 0.0)
        r = np.where(onrow, s["wid"], 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(onrow, mu / np.where(onrow, s["nrm"], 1.0), 0.0)
            hw = np.where(onrow, s["h"][idx, r] * w, 0.0)
            ala = np.where(onrow, al, 0.0)
        Dh_r, D2h_r = Dh[idx, r], D2h[idx, r]                # [B,2], [B,2,2]
        dLfh = np.einsum("bkm,bk->bm", D2h_r, f) + Dh_r @ Df  # sum_k D2h_r[k,m] f_k + Dh_r[k] Df[k,m]
        dLgh = np.einsum("bkm,bk->bm", D2h_r, g)
        with np.errstate(invalid="ignore"):
            add = (-ala * w)[:, None] * Dh_r - w[:, None] * dLfh - (w * s["u"])[:, None] * dLgh
        lamn = lamn + np.where(onrow[:, None], add, 0.0)
        amin = np.where(onrow, np.minimum(amin, np.abs(s["Lgh"][idx, r])), amin)
        # the parameters: W = a row moves with alpha through its right-hand side, W = a bound is the bound itself
        ga = ga - hw
        gl = gl + np.where(onlb, mu, 0.0)
        gu = gu + np.where(onub, mu, 0.0)
        nrow, nlb, nub = nrow + int((hw != 0.0).sum()), nlb + int((onlb & (mu != 0.0)).sum()), nub + int((onub & (mu != 0.0)).sum())
        S = np.maximum(S, np.abs(hw))
        mu = np.where(solved, 0.0, mu)
        S = np.maximum(S, np.abs(lamn).max(axis=1))
        gk = gk + d
        S = np.maximum(S, np.abs(d))
        if gv is not None:
            gv[t, 0] = d
        if K is not None:
            dx = d[None, :] * x                              # [2,B]
            gK = gK + dx
            lamn = lamn + (K * d[None, :]).T
            S = np.maximum(S, np.abs(dx).max(axis=0))
        lam = lamn
        S = np.maximum(S, np.abs(lam).max(axis=1))
    return dict(gx0=lam.T.copy(), gk=gk[None, :].copy(), gK=gK, gv=gv, guact0=mu[None, :].copy(),
                galpha=ga if alpha is not None else None, glb=gl[None, :].copy() if lb is not None else None,
                gub=gu[None, :].copy() if ub is not None else None, nrow=nrow, nlb=nlb, nub=nub, S=S, amin=amin)
