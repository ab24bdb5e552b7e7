"""Reference for the fused explicit rollout and its adjoint (asif_hip_rollout_batch / asif_hip_rollout_vjp_batch on the
double integrator), in numpy.

TEST INFRASTRUCTURE, not a test.  The model (examples/DoubleIntegrator.cpp:12-61), its second derivatives and the
one-variable projection of class ASIF with a pinned relaxation variable are restated here, independently of the product's
headers; tests/test_rollout_vjp_ref_host.py checks the forward pass against the oracle's exact filter and the adjoint
against central differences of that forward pass.

Forward, t = 0 ... T-1, u_{-1} = uact_prev:
    xlog[t] = x_t;  (ok_t, u*_t) = filter(x_t, udes);  u_t = ok_t ? u*_t : u_{t-1};  ulog[t] = u_t;  rclog[t] = +-1
    x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
Adjoint, t = T-1 ... 0, from lambda = gxT, mu = guactT, gudes = 0:
    mu += gulog[t] + dt g' lambda;   lambda' = lambda + dt (Df + u_t Dg)' lambda + gxlog[t]
    rclog[t] == 1:  W = the constraint the projection ended on (none: the unconstrained minimiser), gbar = mu:
                    W empty:  gudes += gbar                                      (2 z = gbar)
                    W = row r (normal a = Lgh_r) or a bound (a = +-1):  w = gbar / a,  z = 0, and for a row
                        lambda' += -relaxLb w Dh_r - w dLfh_r/dx - w u* dLgh_r/dx
                    mu = 0
    otherwise mu passes on.
The sweep runs on GIVEN logs (its own forward pass's, or a device's); rclog decides which steps are solved.
"""
import numpy as np

NX, NU, NP = 2, 1, 4
ACTIVE_TOL = 1e-9  # GiSmall::kActiveTol: a conflict between rows counts beyond this, relative to the row's own terms


def options(oracle, npSSmax=0):
    """The fields of the oracle's default options the explicit class reads, and the oracle's own (model, variant, o)."""
    model, variant = oracle.CONFIGS[2]
    o = oracle.default_options(model, variant)
    o.npSSmax = npSSmax
    keep = npSSmax if 0 < npSSmax < NP else NP
    return dict(lb=float(o.lb[0]), ub=float(o.ub[0]), relaxLb=float(o.relaxLb), keep=keep, oracle=(model, variant, o))


def model(x):
    """x [2,B] -> h [B,4], Dh [B,4,2], D2h [B,4,2,2], f [B,2], g [B,2], Df [2,2] (d f_k / d x_m at [k,m]), Dg = 0."""
    p, v = x[0], x[1]
    B = p.shape[0]
    fwd = v > 0
    brake = (v * v) / 2.0
    h = np.stack([np.where(fwd, 1.0 - p - brake, -p + 1.0), np.where(fwd, p + 1.0, p + 1.0 - brake), v + 1.0, -v + 1.0],
                 axis=1)
    Dh = np.zeros((B, NP, NX))
    Dh[:, 0, 0], Dh[:, 0, 1] = -1.0, np.where(fwd, -v, 0.0)
    Dh[:, 1, 0], Dh[:, 1, 1] = 1.0, np.where(fwd, 0.0, -v)
    Dh[:, 2, 1], Dh[:, 3, 1] = 1.0, -1.0
    D2h = np.zeros((B, NP, NX, NX))
    D2h[:, 0, 1, 1] = np.where(fwd, -1.0, 0.0)
    D2h[:, 1, 1, 1] = np.where(fwd, 0.0, -1.0)
    f = np.stack([v, np.zeros(B)], axis=1)
    g = np.tile(np.array([0.0, 1.0]), (B, 1))
    Df = np.array([[0.0, 1.0], [0.0, 0.0]])
    return h, Dh, D2h, f, g, Df


def filter_step(x, udes, opt):
    """One filter call on x [2,B], udes [B].  Returns a dict: ok [B] bool, u [B] (the clipped point, also where not ok),
    wid [B] (-1 free, 0..3 safety row, 4 lower bound, 5 upper bound), nrm [B] (the normal of W, 0 when free), and the
    model's arrays at x."""
    h, Dh, D2h, f, g, Df = model(x)
    B = udes.shape[0]
    Lfh = np.einsum("brk,bk->br", Dh, f)
    Lgh = np.einsum("brk,bk->br", Dh, g)
    a = Lgh.copy()
    b = -Lfh - h * opt["relaxLb"]
    if opt["keep"] < NP:  # the rows of the `keep` smallest h; ties: lower index first
        pos = np.argsort(np.argsort(h, axis=1, kind="stable"), axis=1, kind="stable")
        drop = pos >= opt["keep"]
        a[drop], b[drop] = 0.0, -1e20
    lb, ub = opt["lb"], opt["ub"]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = b / np.where(a != 0.0, a, 1.0)
    lo = np.maximum(lb, np.where(a > 0.0, q, -np.inf).max(axis=1))
    hi = np.minimum(ub, np.where(a < 0.0, q, np.inf).min(axis=1))
    u = np.minimum(np.maximum(udes, lo), hi)
    t = a * u[:, None]
    bad = ((b - t) > ACTIVE_TOL * (1.0 + np.abs(b) + np.abs(t))).any(axis=1)
    bad |= (lb - u > ACTIVE_TOL * (1.0 + np.abs(u) + abs(lb))) | (u - ub > ACTIVE_TOL * (1.0 + np.abs(u) + abs(ub)))
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
    return dict(ok=~bad, u=np.minimum(np.maximum(u, lb), ub), wid=wid, nrm=nrm, h=h, Dh=Dh, D2h=D2h, f=f, g=g, Df=Df,
                Lgh=Lgh)


def plant_step(x, u, dt):
    """examples/DoubleIntegrator.cpp:96-110, no contraction: fCl = 0 + f + u g;  x += dt fCl."""
    f0, f1 = (0.0 + x[1]) + u * 0.0, (0.0 + 0.0) + u * 1.0
    return np.stack([x[0] + dt * f0, x[1] + dt * f1])


def forward(x0, udes, uact_prev, T, dt, opt):
    """x0 [2,B], udes [1,B], uact_prev [1,B] -> dict xT [2,B], uactT [1,B], xlog [T,2,B], ulog [T,1,B], rclog [T,B]
    int32, wid [T,B] (the working set of each step; -2 where the step failed)."""
    B = x0.shape[1]
    x, u = x0.copy(), uact_prev[0].copy()
    xlog, ulog = np.zeros((T, NX, B)), np.zeros((T, NU, B))
    rclog, wid = np.zeros((T, B), dtype=np.int32), np.zeros((T, B), dtype=int)
    for t in range(T):
        xlog[t] = x
        s = filter_step(x, udes[0], opt)
        u = np.where(s["ok"], s["u"], u)
        ulog[t, 0] = u
        rclog[t] = np.where(s["ok"], 1, -1)
        wid[t] = np.where(s["ok"], s["wid"], -2)
        x = plant_step(x, u, dt)
    return dict(xT=x, uactT=u[None, :].copy(), xlog=xlog, ulog=ulog, rclog=rclog, wid=wid)


def adjoint(xlog, ulog, rclog, udes, dt, opt, gxT, guactT=None, gxlog=None, gulog=None):
    """The sweep on given logs.  Returns dict gx0 [2,B], gudes [1,B], guact0 [1,B], S [B] (largest |lambda| or |mu| met
    along the sweep), amin [B] (smallest |Lgh| of a safety row active at a solved step; 1 if none)."""
    T, _, B = xlog.shape if xlog is not None and len(xlog) else (0, NX, gxT.shape[1])
    lam = gxT.T.copy()                                       # [B,2]
    mu = guactT[0].copy() if guactT is not None else np.zeros(B)
    gudes = np.zeros(B)
    S = np.maximum(np.abs(lam).max(axis=1), np.abs(mu))
    amin = np.ones(B)
    for t in range(T - 1, -1, -1):
        s = filter_step(xlog[t], udes[0], opt)
        Dh, D2h, f, g, Df = s["Dh"], s["D2h"], s["f"], s["g"], s["Df"]
        mu = mu + (gulog[t, 0] if gulog is not None else 0.0) + dt * np.einsum("bk,bk->b", g, lam)
        lamn = lam + dt * (lam @ Df)                         # (Df' lambda)_m = sum_k Df[k,m] lambda_k;  Dg = 0
        if gxlog is not None:
            lamn = lamn + gxlog[t].T
        S = np.maximum(S, np.maximum(np.abs(lamn).max(axis=1), np.abs(mu)))
        solved = rclog[t] == 1
        free = solved & (s["wid"] < 0)
        onrow = solved & (s["wid"] >= 0) & (s["wid"] < NP)
        gudes = gudes + np.where(free, mu, 0.0)
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
        lam = lamn
        S = np.maximum(S, np.abs(lam).max(axis=1))
    return dict(gx0=lam.T.copy(), gudes=gudes[None, :].copy(), guact0=mu[None, :].copy(), S=S, amin=amin)


def census(fw):
    """Counts over the steps of a forward pass: failed, on a safety row, on an input bound, free; and the number of
    instances with both failed and solved steps."""
    wid = fw["wid"]
    failed = wid == -2
    return dict(failed=int(failed.sum()), row=int(((wid >= 0) & (wid < NP)).sum()), bound=int((wid >= NP).sum()),
                free=int((wid == -1).sum()), mixed=int((failed.any(axis=0) & (~failed).any(axis=0)).sum()))
