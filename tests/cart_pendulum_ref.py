"""Reference for class ASIF on the synthetic cart-driven pendulum (ASIF_HIP_MODEL_CART_PENDULUM): the explicit filter, the
fused rollout under an affine policy with the barrier gain and the input box per instance, and its adjoint, in numpy.

TEST INFRASTRUCTURE, not a test.  The oracle has no such model: everything is restated here, independently of the product's
headers, and tests/test_cart_pendulum_ref_host.py checks the adjoint against central differences of the forward pass
before anything on the device is compared with it.

Model, x = (theta, omega), one input:
    f = (omega, sin theta)          g = (0, -cos theta)
    Df = [[0, 1], [cos theta, 0]]   Dg: d g_1 / d theta = sin theta, every other entry 0
    fwd = omega > 0
    h0 = fwd ? 1 - theta - omega^2/2 : 1 - theta          h1 = fwd ? theta + 1 : theta + 1 - omega^2/2
    h2 = 1.5 - (theta^2 + theta omega + omega^2)          h3 = cos theta - omega^2/2
Forward, t = 0 ... T-1, u_{-1} = uact_prev:
    uDes_t = k + K x_t + v_t
    (ok_t, u*_t) = the projection of uDes_t onto  { Lgh_r u >= -Lfh_r - alpha_i h_r,  lb_i <= u <= ub_i }
    u_t = ok_t ? u*_t : u_{t-1};   x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
Adjoint, t = T-1 ... 0, from lambda = gxT, mu = guactT:
    mu += gulog[t] + dt g' lambda;   lambda' = lambda + dt (Df + u_t Dg)' lambda + gxlog[t]
    rclog[t] == 1, W the constraint the projection ended on, w = mu / its normal:
        W empty:  d_t = mu
        W = row r:  lambda' += -alpha w Dh_r - w dLfh_r/dx - w u* dLgh_r/dx,   galpha += -h_r w
                    dLfh_r/dx_m = sum_k D2h_r[k,m] f_k + Dh_r[k] Df[k,m]
                    dLgh_r/dx_m = sum_k D2h_r[k,m] g_k + Dh_r[k] Dg[k,m]
        W = a bound:  glb += mu  /  gub += mu
        mu = 0
    gk += d_t;  gK[m] += d_t x_t[m];  gv[t] = d_t;  lambda' += K' d_t
LINEARISED (the switch of adjoint): Dg and the mixed entries of D2h are taken as zero -- what a sweep written for the double
integrator alone would compute; the sensitivity test shows that the suite sees the difference.
"""
import numpy as np

NX, NU, NP = 2, 1, 4
ACTIVE_TOL = 1e-9  # GiSmall::kActiveTol: a conflict between rows counts beyond this, relative to the row's own terms
MODEL = 10         # ASIF_HIP_MODEL_CART_PENDULUM


def options(npSSmax=0):
    """asif_hip_default_options(10, EXPLICIT): the class defaults with the input box [-4, 4]."""
    keep = npSSmax if 0 < npSSmax < NP else NP
    return dict(lb=-4.0, ub=4.0, relaxLb=5.0, relaxCost=50.0, keep=keep)


def model(x, linearised=False):
    """x [2,B] -> h [B,4], Dh [B,4,2], D2h [B,4,2,2], f [B,2], g [B,2], Df [B,2,2] (d f_k / d x_m at [k,m]),
    Dg [B,2,2] (d g_k / d x_m at [k,m])."""
    th, om = x[0], x[1]
    B = th.shape[0]
    s, c = np.sin(th), np.cos(th)
    fwd = om > 0
    brake = (om * om) / 2.0
    h = np.stack([np.where(fwd, 1.0 - th - brake, -th + 1.0), np.where(fwd, th + 1.0, th + 1.0 - brake),
                  1.5 - ((th * th + th * om) + om * om), c - brake], axis=1)
    Dh = np.zeros((B, NP, NX))
    Dh[:, 0, 0], Dh[:, 0, 1] = -1.0, np.where(fwd, -om, 0.0)
    Dh[:, 1, 0], Dh[:, 1, 1] = 1.0, np.where(fwd, 0.0, -om)
    Dh[:, 2, 0], Dh[:, 2, 1] = -(2.0 * th + om), -(th + 2.0 * om)
    Dh[:, 3, 0], Dh[:, 3, 1] = -s, -om
    D2h = np.zeros((B, NP, NX, NX))
    D2h[:, 0, 1, 1] = np.where(fwd, -1.0, 0.0)
    D2h[:, 1, 1, 1] = np.where(fwd, 0.0, -1.0)
    D2h[:, 2, 0, 0], D2h[:, 2, 1, 1] = -2.0, -2.0
    D2h[:, 2, 0, 1], D2h[:, 2, 1, 0] = -1.0, -1.0
    D2h[:, 3, 0, 0], D2h[:, 3, 1, 1] = -c, -1.0
    f = np.stack([om, s], axis=1)
    g = np.stack([np.zeros(B), -c], axis=1)
    Df = np.zeros((B, NX, NX))
    Df[:, 0, 1], Df[:, 1, 0] = 1.0, c
    Dg = np.zeros((B, NX, NX))
    Dg[:, 1, 0] = s
    if linearised:
        Dg[:] = 0.0
        D2h[:, :, 0, 1] = D2h[:, :, 1, 0] = 0.0
    return h, Dh, D2h, f, g, Df, Dg


def rows(x, keep=NP):
    """The class's rows at x [2,B] as asif_hip_assemble_batch hands them out: A [keep*2,B] (Lgh of row p at component p,
    h at p + keep), b [keep,B] = -Lfh, which [keep,B] the safety function in each row (ascending h, ties: lower index)."""
    h, Dh, _, f, g, _, _ = model(x)
    Lfh = np.einsum("brk,bk->br", Dh, f)
    Lgh = np.einsum("brk,bk->br", Dh, g)
    order = np.argsort(h, axis=1, kind="stable")[:, :keep] if keep < NP else np.tile(np.arange(NP), (h.shape[0], 1))
    take = lambda a: np.take_along_axis(a, order, axis=1).T
    return np.concatenate([take(Lgh), take(h)]), -take(Lfh), order.T


def lane_params(opt, B, alpha=None, lb=None, ub=None):
    """alpha [B], lb [B], ub [B] (lb / ub handed in as [1,B]) and gain_ok [B]: the handle's value where None."""
    full = lambda v: np.full(B, float(v))
    al = full(opt["relaxLb"]) if alpha is None else np.asarray(alpha, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.ones(B, dtype=bool) if alpha is None else (al > 0.0) & (al < np.inf)
    return (al, full(opt["lb"]) if lb is None else np.asarray(lb[0], dtype=np.float64),
            full(opt["ub"]) if ub is None else np.asarray(ub[0], dtype=np.float64), ok)


def filter_step(x, udes, keep, al, lb, ub, gain_ok, linearised=False, lie=None):
    """One filter call on x [2,B], udes [B] with alpha, lb, ub [B].  Returns a dict: ok [B] bool, u [B] (the clipped
    point, also where not ok), wid [B] (-1 free, 0..3 safety row, 4 lower bound, 5 upper bound), nrm [B] (the normal of
    W, 0 when free), margin [B] (how far the feasibility test is from its threshold, relative to the threshold's own
    terms; small: the verdict may turn on the last bits of sin / cos), and the model's arrays at x.
    lie: (lfh [keep,B], lgh [keep,B]) caller-supplied Lie derivatives, indexed by row position (ascending h)."""
    h, Dh, D2h, f, g, Df, Dg = model(x, linearised)
    B = udes.shape[0]
    Lfh = np.einsum("brk,bk->br", Dh, f)
    Lgh = np.einsum("brk,bk->br", Dh, g)
    pos = np.argsort(np.argsort(h, axis=1, kind="stable"), axis=1, kind="stable") if keep < NP else np.tile(np.arange(NP), (B, 1))
    if lie is not None:
        p = np.where(pos < keep, pos, 0)
        Lfh, Lgh = np.take_along_axis(lie[0].T, p, axis=1), np.take_along_axis(lie[1].T, p, axis=1)
    a = Lgh.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b = -Lfh - h * al[:, None]
        drop = pos >= keep
        a[drop], b[drop] = 0.0, -1e20
        q = b / np.where(a != 0.0, a, 1.0)
        lo = np.fmax(lb, np.where(a > 0.0, q, -np.inf).max(axis=1))
        hi = np.fmin(ub, np.where(a < 0.0, q, np.inf).min(axis=1))
        u = np.fmin(np.fmax(udes, lo), hi)
        t = a * u[:, None]
        viol = np.concatenate([(b - t) - ACTIVE_TOL * (1.0 + np.abs(b) + np.abs(t)),
                               ((lb - u) - ACTIVE_TOL * (1.0 + np.abs(u) + np.abs(lb)))[:, None],
                               ((u - ub) - ACTIVE_TOL * (1.0 + np.abs(u) + np.abs(ub)))[:, None]], axis=1)
        size = np.concatenate([1.0 + np.abs(b) + np.abs(t), (1.0 + np.abs(u) + np.abs(lb))[:, None],
                               (1.0 + np.abs(u) + np.abs(ub))[:, None]], axis=1)
        bad = (viol > 0.0).any(axis=1)
        margin = np.abs(viol / size).min(axis=1)
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
    return dict(ok=~bad, u=uc, wid=wid, nrm=nrm, margin=margin, h=h, Dh=Dh, D2h=D2h, f=f, g=g, Df=Df, Dg=Dg, Lgh=Lgh,
                pos=pos)


def policy(k, K, v_t, x):
    """uDes_t [B] in the one evaluation order: k, + K[m] x[m] for m = 0 ... nx-1, + v_t."""
    u = k[0].copy()
    if K is not None:
        for m in range(NX):
            u = u + K[m] * x[m]
    if v_t is not None:
        u = u + v_t[0]
    return u


def plant_step(x, u, dt):
    """The kernels' Euler step, no contraction: fCl = 0 + f + u g;  x += dt fCl."""
    f0, f1 = (0.0 + x[1]) + u * 0.0, (0.0 + np.sin(x[0])) + u * (-np.cos(x[0]))
    return np.stack([x[0] + dt * f0, x[1] + dt * f1])


def forward(x0, k, K, v, uact_prev, T, dt, opt, alpha=None, lb=None, ub=None):
    """x0 [2,B], k [1,B], K [2,B] or None, v [T,1,B] or None, uact_prev [1,B], alpha [B], lb, ub [1,B] (each or None: the
    handle's value) -> dict xT, uactT, xlog [T,2,B], ulog [T,1,B], rclog [T,B] int32, wid [T,B] (the working set of each
    step; -2 where the step failed), udes [T,B]."""
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


def adjoint(xlog, ulog, rclog, k, K, v, dt, opt, gxT, guactT=None, gxlog=None, gulog=None, alpha=None, lb=None, ub=None,
            linearised=False):
    """The sweep on given logs.  Returns dict gx0 [2,B], gk [1,B], gK [2,B] (None without K), gv [T,1,B] (None without v),
    guact0 [1,B], galpha [B], glb [1,B], gub [1,B] (each None where the parameter is None), nrow / nlb / nub (steps with a
    nonzero contribution to each), S [B] (the largest magnitude among lambda, mu, d_t, d_t x_t' and h_r w_r along the
    sweep), amin [B] (smallest |Lgh| of a safety row active at a solved step; 1 if none)."""
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
        s = filter_step(x, policy(k, K, None if v is None else v[t], x), opt["keep"], *par, linearised=linearised)
        Dh, D2h, f, g, Df, Dg = s["Dh"], s["D2h"], s["f"], s["g"], s["Df"], s["Dg"]
        mu = mu + (gulog[t, 0] if gulog is not None else 0.0) + dt * np.einsum("bk,bk->b", g, lam)
        J = Df + ulog[t, 0][:, None, None] * Dg              # d (f + g u_t)_k / d x_m at [k,m]
        lamn = lam + dt * np.einsum("bkm,bk->bm", J, lam)
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
        dLfh = np.einsum("bkm,bk->bm", D2h_r, f) + np.einsum("bk,bkm->bm", Dh_r, Df)
        dLgh = np.einsum("bkm,bk->bm", D2h_r, g) + np.einsum("bk,bkm->bm", Dh_r, Dg)
        with np.errstate(invalid="ignore"):
            add = (-ala * w)[:, None] * Dh_r - w[:, None] * dLfh - (w * s["u"])[:, None] * dLgh
        lamn = lamn + np.where(onrow[:, None], add, 0.0)
        amin = np.where(onrow, np.minimum(amin, np.abs(s["Lgh"][idx, r])), amin)
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


def filter_vjp(x, udes, gbar, opt, lie=None):
    """The one-step adjoint of the filter (asif_hip_filter_vjp_batch) at gbar [B] = dL/duAct: dict rc [B] (1 / -1),
    gudes [1,B], smin [B] (|normal| of W; 1 when free), margin [B] and, with caller-supplied Lie derivatives
    lie = (lfh [keep,B], lgh [keep,B]), glfh [keep,B], glgh [keep,B] (by row position) and gx [2,B] (through h alone)."""
    B = udes.shape[0]
    keep = opt["keep"]
    s = filter_step(x, udes, keep, *lane_params(opt, B), lie=lie)
    ok = s["ok"]
    free, onrow = ok & (s["wid"] < 0), ok & (s["wid"] >= 0) & (s["wid"] < NP)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(onrow, gbar / np.where(onrow, s["nrm"], 1.0), 0.0)
    out = dict(rc=np.where(ok, 1, -1).astype(np.int32), gudes=np.where(free, gbar, 0.0)[None, :], margin=s["margin"],
               smin=np.where(ok & (s["wid"] >= 0), np.abs(np.where(s["nrm"] != 0.0, s["nrm"], 1.0)), 1.0), wid=s["wid"])
    if lie is not None:
        r = np.where(onrow, s["wid"], 0)
        p = s["pos"][np.arange(B), r]
        glfh, glgh = np.zeros((keep, B)), np.zeros((keep, B))
        at = np.flatnonzero(onrow)
        glfh[p[at], at] = -w[at]
        glgh[p[at], at] = -w[at] * s["u"][at]
        out.update(glfh=glfh, glgh=glgh, gx=(-opt["relaxLb"] * w)[None, :] * s["Dh"][np.arange(B), r].T)
    return out


def census(fw):
    """Counts over the steps of a forward pass: failed, on a safety row, on an input bound, free; and the number of
    instances with both failed and solved steps."""
    wid = fw["wid"]
    failed = wid == -2
    return dict(failed=int(failed.sum()), row=int(((wid >= 0) & (wid < NP)).sum()), bound=int((wid >= NP).sum()),
                free=int((wid == -1).sum()), mixed=int((failed.any(axis=0) & (~failed).any(axis=0)).sum()))
