"""Reference for the fused explicit rollout under an affine policy and its adjoint (asif_hip_rollout_policy_batch /
asif_hip_rollout_policy_vjp_batch on the double integrator), in numpy.

TEST INFRASTRUCTURE, not a test.  The model, the filter's one-variable projection and the plant step are those of
tests/rollout_vjp_ref.py; this file adds the policy and the routing of each step's d_t = dL/duDes_t.

Forward, t = 0 ... T-1, u_{-1} = uact_prev:
    uDes_t = k + K x_t + v_t  (k, then K[0,m] x_m for m = 0, 1, then v_t; an absent term is not evaluated)
    xlog[t] = x_t;  (ok_t, u*_t) = filter(x_t, uDes_t);  u_t = ok_t ? u*_t : u_{t-1};  ulog[t] = u_t;  rclog[t] = +-1
    x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
Adjoint, t = T-1 ... 0: the sweep of rollout_vjp_ref.adjoint, with the step's d_t (mu on a step that ends free, zero on a
failed step and on one that ends on a row or a bound) distributed as
    gk += d_t;   gK[m] += d_t x_t[m];   gv[t] = d_t;   lambda += K' d_t   (lambda: the value the step leaves for t-1)
K [2,B] holds the gain's entry (0, m) at component m (nu = 1: component j + m nu), v [T,1,B].
"""
import numpy as np

from rollout_vjp_ref import NP, NU, NX, filter_step, model, options, plant_step  # noqa: F401  (re-exported)


def policy(k, K, v_t, x):
    """uDes_t [B] in the one evaluation order: k, + K[m] x[m] for m = 0 ... nx-1, + v_t."""
    u = k[0].copy()
    if K is not None:
        for m in range(NX):
            u = u + K[m] * x[m]
    if v_t is not None:
        u = u + v_t[0]
    return u


def forward(x0, k, K, v, uact_prev, T, dt, opt):
    """x0 [2,B], k [1,B], K [2,B] or None, v [T,1,B] or None, uact_prev [1,B] -> dict xT, uactT, xlog [T,2,B],
    ulog [T,1,B], rclog [T,B] int32, wid [T,B] (the working set of each step; -2 where the step failed), udes [T,B]."""
    B = x0.shape[1]
    x, u = x0.copy(), uact_prev[0].copy()
    xlog, ulog, udl = np.zeros((T, NX, B)), np.zeros((T, NU, B)), np.zeros((T, B))
    rclog, wid = np.zeros((T, B), dtype=np.int32), np.zeros((T, B), dtype=int)
    for t in range(T):
        xlog[t] = x
        udl[t] = policy(k, K, None if v is None else v[t], x)
        s = filter_step(x, udl[t], opt)
        u = np.where(s["ok"], s["u"], u)
        ulog[t, 0] = u
        rclog[t] = np.where(s["ok"], 1, -1)
        wid[t] = np.where(s["ok"], s["wid"], -2)
        x = plant_step(x, u, dt)
    return dict(xT=x, uactT=u[None, :].copy(), xlog=xlog, ulog=ulog, rclog=rclog, wid=wid, udes=udl)


def adjoint(xlog, ulog, rclog, k, K, v, dt, opt, gxT, guactT=None, gxlog=None, gulog=None):
    """The sweep on given logs.  Returns dict gx0 [2,B], gk [1,B], gK [2,B] (None without K), gv [T,1,B] (None without v),
    guact0 [1,B], S [B] (the largest magnitude among lambda, mu, d_t and d_t x_t' along the sweep), amin [B] (smallest
    |Lgh| of a safety row active at a solved step; 1 if none)."""
    T, _, B = xlog.shape if xlog is not None and len(xlog) else (0, NX, gxT.shape[1])
    lam = gxT.T.copy()                                       # [B,2]
    mu = guactT[0].copy() if guactT is not None else np.zeros(B)
    gk = np.zeros(B)
    gK = np.zeros((NX, B)) if K is not None else None
    gv = np.zeros((T, NU, B)) if v is not None else None
    S = np.maximum(np.abs(lam).max(axis=1), np.abs(mu))
    amin = np.ones(B)
    for t in range(T - 1, -1, -1):
        x = xlog[t]
        s = filter_step(x, policy(k, K, None if v is None else v[t], x), opt)
        Dh, D2h, f, g, Df = s["Dh"], s["D2h"], s["f"], s["g"], s["Df"]
        mu = mu + (gulog[t, 0] if gulog is not None else 0.0) + dt * np.einsum("bk,bk->b", g, lam)
        lamn = lam + dt * (lam @ Df)                         # (Df' lambda)_m = sum_k Df[k,m] lambda_k;  Dg = 0
        if gxlog is not None:
            lamn = lamn + gxlog[t].T
        S = np.maximum(S, np.maximum(np.abs(lamn).max(axis=1), np.abs(mu)))
        solved = rclog[t] == 1
        free = solved & (s["wid"] < 0)
        onrow = solved & (s["wid"] >= 0) & (s["wid"] < NP)
        d = np.where(free, mu, 0.0)
        r = np.where(onrow, s["wid"], 0)
        idx = np.arange(B)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(onrow, mu / np.where(onrow, s["nrm"], 1.0), 0.0)
        Dh_r, D2h_r = Dh[idx, r], D2h[idx, r]                # [B,2], [B,2,2]
        dLfh = np.einsum("bkm,bk->bm", D2h_r, f) + Dh_r @ Df  # sum_k D2h_r[k,m] f_k + Dh_r[k] Df[k,m]
        dLgh = np.einsum("bkm,bk->bm", D2h_r, g)
        add = (-opt["relaxLb"] * w)[:, None] * Dh_r - w[:, None] * dLfh - (w * s["u"])[:, None] * dLgh
        lamn = lamn + np.where(onrow[:, None], add, 0.0)
        amin = np.where(onrow, np.minimum(amin, np.abs(s["Lgh"][idx, r])), amin)
        mu = np.where(solved, 0.0, mu)
        S = np.maximum(S, np.abs(lamn).max(axis=1))
        # the policy: d_t to k, K, v_t and, through K, back into the state gradient
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
    return dict(gx0=lam.T.copy(), gk=gk[None, :].copy(), gK=gK, gv=gv, guact0=mu[None, :].copy(), S=S, amin=amin)


def census(fw):
    """Counts over the steps of a forward pass: failed, on a safety row, on an input bound, free; and the number of
    instances with both failed and solved steps."""
    wid = fw["wid"]
    failed = wid == -2
    return dict(failed=int(failed.sum()), row=int(((wid >= 0) & (wid < NP)).sum()), bound=int((wid >= NP).sum()),
                free=int((wid == -1).sum()), mixed=int((failed.any(axis=0) & (~failed).any(axis=0)).sum()))
