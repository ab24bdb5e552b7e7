"""Problems and reference for the QP solve's vector-Jacobian product (asif_hip_qp_vjp_batch), in numpy.

TEST INFRASTRUCTURE, not a test.  family() draws seeded, feasible problems of one shape; adjoint() works from the exact
optimum of the CPU oracle (oracle.qp_solve_batch(..., SOLVER_EXACT)):

    min x'Hx + c'x   s.t.  A x >= b (== b where be),  lb <= x <= ub,   D = 2H
    candidates: the nc rows (a_k, b_k), the lower bounds (+e_j, lb_j), the upper bounds (-e_j, -ub_j); a variable with
                lb == ub counts once, as its lower bound
    W  = every candidate with |slack| <= 1e-9 at x*,  N = their normals
    lambda: least squares  N' lambda = 2 H x* + c
    adjoint:  D z + N' w = gsol,  N z = 0   ->   w: least squares on N D^-1/2,  z = D^-1 (gsol - N' w)   (|W| = nv: z = 0)
    gc = -z;  gHd_j = -2 x*_j z_j;  k in W:  gb_k = w_k,  gA_k = lambda_k z' - w_k x*';  glb_j = w;  gub_j = -w

An instance is flagged `degenerate` (the derivative is one-sided, or the active set is not what a solver must find) when
some inactive slack is < 1e-5, some inequality multiplier is < 1e-6, or |W| > nv.  smin = sigma_min of N D^-1/2 (1 for
an empty W).
"""
import zlib

import numpy as np

ACTIVE_TOL, NEAR_TOL, WEAK_TOL = 1e-9, 1e-5, 1e-6
KINDS = ("plain", "pinned", "eqrow")
GRADS = ("gHd", "gc", "gA", "gb", "glb", "gub")


def family(nv, nc, kind, B):
    """AoS, as the oracle takes them: Hd, c, lb, ub [B,nv]; A [B,nv*nc] (entry (r, j) at r + j*nc); b [B,nc];
    be uint8[nc]; gsol [B,nv].  Feasible by construction: an interior point p with slacks s."""
    rng = np.random.default_rng(zlib.crc32(f"qpvjp:{nv}x{nc}:{kind}".encode()))
    Hd = np.exp(rng.uniform(np.log(0.5), np.log(4.0), (B, nv)))
    c = rng.normal(0, 6, (B, nv))
    A = rng.normal(0, 1, (B, nv, nc))
    lb = -rng.uniform(0.5, 3, (B, nv))
    ub = rng.uniform(0.5, 3, (B, nv))
    p = rng.uniform(-0.4, 0.4, (B, nv))
    s = rng.uniform(0.05, 1.5, (B, nc))
    be = np.zeros(nc, dtype=np.uint8)
    if kind == "pinned":
        lb[:, -1] = ub[:, -1] = p[:, -1] = rng.uniform(1, 6, B)
    elif kind == "eqrow":
        be[0] = 1
        s[:, 0] = 0.0
    elif kind != "plain":
        raise ValueError(kind)
    b = np.einsum("bjr,bj->br", A, p) - s
    gsol = rng.normal(0, 1, (B, nv))
    return dict(nv=nv, nc=nc, kind=kind, Hd=Hd, c=c, A=np.ascontiguousarray(A.reshape(B, nv * nc)), b=b, lb=lb, ub=ub,
                be=be, gsol=gsol)


def solve(oracle, q):
    """x* [B,nv] and status [B] of the oracle's exact solver."""
    sol, st, _ = oracle.qp_solve_batch(q["nv"], q["nc"], q["Hd"], q["c"], q["A"], q["b"], q["lb"], q["ub"], q["be"],
                                       oracle.SOLVER_EXACT)
    return sol, st


def adjoint(oracle, q):
    """dict of AoS arrays: rc [B] (1 solved, -1 otherwise), sol [B,nv], gHd, gc, glb, gub [B,nv], gA [B,nv*nc],
    gb [B,nc] (zero where rc != 1), and per instance nactive, degenerate, smin."""
    nv, nc = q["nv"], q["nc"]
    B = q["c"].shape[0]
    sol, st = solve(oracle, q)
    ok = st == 1
    x = np.where(ok[:, None], sol, 0.0)
    D = 2.0 * q["Hd"]
    eye = np.eye(nv)
    Arow = q["A"].reshape(B, nv, nc).transpose(0, 2, 1)  # [B, nc, nv]
    N = np.concatenate([Arow, np.tile(eye, (B, 1, 1)), np.tile(-eye, (B, 1, 1))], axis=1)  # [B, nc + 2 nv, nv]
    rhs = np.concatenate([q["b"], q["lb"], -q["ub"]], axis=1)
    slack = np.einsum("bkj,bj->bk", N, x) - rhs
    pinned = q["lb"] == q["ub"]
    slack[:, nc + nv:][pinned] = np.inf  # counted once, as the lower bound
    equality = np.concatenate([np.tile(q["be"] != 0, (B, 1)), pinned, np.zeros((B, nv), dtype=bool)], axis=1)
    act = np.abs(slack) <= ACTIVE_TOL
    m = act.sum(axis=1)
    deg = (m > nv) | ((slack < NEAR_TOL) & ~act).any(axis=1)
    out = dict(rc=np.where(ok, 1, -1).astype(np.int32), sol=sol, nactive=np.where(ok, m, 0), smin=np.ones(B))
    for k, n in (("gHd", nv), ("gc", nv), ("gA", nv * nc), ("gb", nc), ("glb", nv), ("gub", nv)):
        out[k] = np.zeros((B, n))
    kkt = D * x + q["c"]
    z = q["gsol"] / D
    order = np.argsort(~act, axis=1, kind="stable")  # active candidates first, in increasing id
    for mm in range(1, nv + 1):
        I = np.where(ok & (m == mm))[0]
        if not len(I):
            continue
        W = order[I, :mm]
        NW = np.take_along_axis(N[I], W[:, :, None], 1)  # [n, mm, nv]
        NWt = NW.transpose(0, 2, 1)
        lam = np.einsum("nkj,nj->nk", np.linalg.pinv(NWt), kkt[I])
        ineq = ~np.take_along_axis(equality[I], W, 1)
        deg[I] |= ((lam < WEAK_TOL) & ineq).any(axis=1)
        S = NW / np.sqrt(D[I])[:, None, :]
        out["smin"][I] = np.linalg.svd(S, compute_uv=False).min(axis=1)
        if mm == nv:
            w = np.linalg.solve(NWt, q["gsol"][I][:, :, None])[:, :, 0]
            z[I] = 0.0  # N_W spans everything: the null-space part is zero, not rounding
        else:
            w = np.einsum("nkj,nj->nk", np.linalg.pinv(S.transpose(0, 2, 1)), q["gsol"][I] / np.sqrt(D[I]))
            z[I] = (q["gsol"][I] - np.einsum("nkj,nk->nj", NW, w)) / D[I]
        for t in range(mm):
            k, wt, lt = W[:, t], w[:, t], lam[:, t]
            row = k < nc
            Ir, kr = I[row], k[row]
            out["gb"][Ir, kr] = wt[row]
            for j in range(nv):
                out["gA"][Ir, kr + j * nc] = lt[row] * z[Ir, j] - wt[row] * x[Ir, j]
            lo = (k >= nc) & (k < nc + nv)
            out["glb"][I[lo], k[lo] - nc] = wt[lo]
            up = k >= nc + nv
            out["gub"][I[up], k[up] - nc - nv] = -wt[up]
    z = np.where(ok[:, None], z, 0.0)
    out["gc"] = -z
    out["gHd"] = -2.0 * x * z
    out["degenerate"] = deg & ok
    return out
