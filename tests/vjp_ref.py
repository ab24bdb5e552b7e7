"""Reference for the explicit filter's vector-Jacobian product (asif_hip_filter_vjp_batch), in numpy.

TEST INFRASTRUCTURE, not a test.  Works from what the CPU oracle provides: the rows of oracle.assemble_batch
(caller-supplied lfh / lgh substituted where given) and the exact optimum u*, rc of oracle.filter_batch /
oracle.filter_explicit_lie.  Per solved instance:

    u* = projection of uDes onto {G u >= r, lb <= u <= ub},  G = Lgh,  r = -Lfh - h relaxLb
    W  = every row or bound with |slack| <= 1e-9 at u* (bounds as rows +-e_j),  N = their normals
    lambda: least squares  N' lambda = 2 (u* - uDes)
    adjoint:  2 z + N' w = gbar,  N z = 0   ->   w = (N N')^-1 N gbar,  z = (gbar - N' w) / 2
    dL/duDes = 2 z;  rows k in W:  dL/dLfh_k = -w_k,  dL/dLgh_k = lambda_k z' - w_k u*',  dL/dh_k = -relaxLb w_k;
    dL/dx = Dh' dL/dh  (x through h alone: lfh and lgh are the caller's)

An instance is flagged `degenerate` (the derivative is one-sided or the active set is not what a solver must find)
when some inactive slack is < 1e-5, some active multiplier is < 1e-6, or |W| > nu.

The oracle hands out h but not Dh; the two models' safety sets are restated here (examples/DoubleIntegrator.cpp:24-38
and the synthetic two-input model of asif_amd/csrc/models.hpp) and h is checked against the oracle's rows.
"""
import numpy as np

ACTIVE_TOL, NEAR_TOL, WEAK_TOL = 1e-9, 1e-5, 1e-6


def safety(cfg, x):
    """h [B,np], Dh [B,np,nx] of config cfg (2: DoubleIntegrator, 11: PlanarTwoInput) for x [B,nx]."""
    B = x.shape[0]
    if cfg == 2:
        p, v = x[:, 0], x[:, 1]
        fwd = v > 0
        brake = v * v / 2.0
        h = np.stack([np.where(fwd, 1.0 - p - brake, -p + 1.0), np.where(fwd, p + 1.0, p + 1.0 - brake), v + 1.0,
                      -v + 1.0], axis=1)
        Dh = np.zeros((B, 4, 2))
        Dh[:, 0, 0], Dh[:, 0, 1] = -1.0, np.where(fwd, -v, 0.0)
        Dh[:, 1, 0], Dh[:, 1, 1] = 1.0, np.where(fwd, 0.0, -v)
        Dh[:, 2, 1], Dh[:, 3, 1] = 1.0, -1.0
        return h, Dh
    if cfg == 11:
        a = np.array([[1., 0.], [-1., 0.], [0., 1.], [0., -1.], [0.6, 0.8]])
        r = np.array([1., 1., 1., 1., 1.2])
        return r[None, :] - x @ a.T, np.tile(-a, (B, 1, 1))
    raise ValueError(cfg)


def rows(oracle, cfg, x, lie=None, npSSmax=0):
    """G [B,nc,nu], Lfh [B,nc], h [B,nc], Dh [B,nc,nx] in row order, and the oracle's options / dims.  x [B,nx] AoS;
    lie = (lfh [nc,B], lgh [nc*nu,B]) or None."""
    model, variant = oracle.CONFIGS[cfg]
    o = oracle.default_options(model, variant)
    o.npSSmax = npSSmax
    d = oracle.dims(model, variant, o)
    B = x.shape[0]
    A, b, _, _ = oracle.assemble_batch(model, variant, o, np.ascontiguousarray(x))
    A = A.reshape(B, d.nv, d.nc).transpose(0, 2, 1).copy()  # [B, nc, nv]
    G, h, Lfh = A[:, :, :d.nu].copy(), A[:, :, d.nu].copy(), -b
    hall, Dhall = safety(cfg, x)
    order = np.argsort(hall, axis=1, kind="stable")[:, :d.nc] if d.nc < d.npSS else np.tile(np.arange(d.nc), (B, 1))
    assert np.allclose(np.take_along_axis(hall, order, 1), h, rtol=0, atol=1e-12), "safety-set restatement != oracle"
    Dh = np.take_along_axis(Dhall, order[:, :, None], 1)
    if lie is not None:
        G = lie[1].T.reshape(B, d.nu, d.nc).transpose(0, 2, 1).copy()
        Lfh = lie[0].T.copy()
    return G, Lfh, h, Dh, o, d


def solve(oracle, cfg, x, udes, lie=None, npSSmax=0):
    """u* [B,nu], rc [B] of the oracle's exact filter."""
    model, variant = oracle.CONFIGS[cfg]
    o = oracle.default_options(model, variant)
    o.npSSmax = npSSmax
    d = oracle.dims(model, variant, o)
    B = x.shape[0]
    if lie is None:
        ua, _, rc = oracle.filter_batch(model, variant, o, np.ascontiguousarray(x), np.ascontiguousarray(udes),
                                        uact_init=np.zeros((B, d.nu)))
    else:
        ua, _, rc = oracle.filter_explicit_lie(model, o, np.ascontiguousarray(x), np.ascontiguousarray(udes),
                                               np.ascontiguousarray(lie[0].T), np.ascontiguousarray(lie[1].T))
    return ua, rc


def vjp(oracle, cfg, x, udes, gbar, lie=None, npSSmax=0):
    """x [nx,B], udes [nu,B], gbar [nu,B] (SoA, as the product takes them).  Returns a dict of SoA arrays: rc [B],
    gudes [nu,B], glfh [nc,B], glgh [nc*nu,B], gx [nx,B] (zero where rc != 1), and per instance nactive, degenerate,
    smin (= sigma_min of the active normals, 1 for an empty set).  glfh / glgh / gx are meaningful on the
    caller-supplied path only (on the model path x also moves Lfh and Lgh)."""
    xa, ud, gb = (np.ascontiguousarray(a.T) for a in (x, udes, gbar))
    G, Lfh, h, Dh, o, d = rows(oracle, cfg, xa, lie, npSSmax)
    ua, rc = solve(oracle, cfg, xa, ud, lie, npSSmax)
    B, nu, nc, nx = xa.shape[0], d.nu, d.nc, d.nx
    lb, ub = np.array(list(o.lb)[:nu]), np.array(list(o.ub)[:nu])
    r = -Lfh - h * o.relaxLb
    out = dict(rc=rc, gudes=np.zeros((nu, B)), glfh=np.zeros((nc, B)), glgh=np.zeros((nc * nu, B)),
               gx=np.zeros((nx, B)), nactive=np.zeros(B, dtype=int), degenerate=np.zeros(B, dtype=bool),
               smin=np.ones(B), uact=ua.T.copy())
    eye = np.eye(nu)
    for i in np.where(rc == 1)[0]:
        N = np.concatenate([G[i], eye, -eye])
        rhs = np.concatenate([r[i], lb, -ub])
        slack = N @ ua[i] - rhs
        act = np.abs(slack) <= ACTIVE_TOL
        W = np.where(act)[0]
        out["nactive"][i] = len(W)
        deg = bool((slack[~act] < NEAR_TOL).any()) or len(W) > nu
        z = 0.5 * gb[i]
        if len(W):
            NW = N[W]
            lam = np.linalg.lstsq(NW.T, 2.0 * (ua[i] - ud[i]), rcond=None)[0]
            deg = deg or bool((lam < WEAK_TOL).any())
            out["smin"][i] = np.linalg.svd(NW, compute_uv=False).min()
            w = np.linalg.lstsq(NW.T, gb[i], rcond=None)[0] if len(W) >= nu else np.linalg.solve(NW @ NW.T, NW @ gb[i])
            z = 0.5 * (gb[i] - NW.T @ w)
            if len(W) >= nu:
                z = np.zeros(nu)  # N_W spans everything: the null-space part is zero, not rounding
            for k, wk, lk in zip(W, w, lam):
                if k < nc:
                    out["glfh"][k, i] = -wk
                    out["glgh"][k::nc, i] = lk * z - wk * ua[i]
                    out["gx"][:, i] += Dh[i, k] * (-o.relaxLb * wk)
        out["gudes"][:, i] = 2.0 * z
        out["degenerate"][i] = deg
    return out
