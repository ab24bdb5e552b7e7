// qp_vjp_small.hpp -- the adjoint of one small QP at the working set its dual active-set solve ended with
// (gi_small.hpp: GiSmall::solve_general<true>), in registers, for nv <= 3 variables and a diagonal cost.
//
//     min x'Hx + c'x   s.t.  A x >= b (== b where be),  lb <= x <= ub,   H = diag(Hd) > 0.
//
// W is the final working set: a general row k has normal a_k and right side b_k, a lower bound normal +e_j and right
// side lb_j, an upper bound normal -e_j and right side -ub_j; |W| <= nv, N its normals, lambda its multipliers
// (2 H x* + c = N' lambda).  With gsol = dL/dx* of a scalar loss L and D = 2H, the adjoint system
//     D z + N' w = gsol,   N z = 0        w = (N D^-1 N')^-1 N D^-1 gsol,   z = D^-1 (gsol - N' w)
// gives
//     dL/dc = -z,   dL/dHd_j = -2 x*_j z_j,
//     k in W:  dL/db_k = w_k,  dL/dA_k = lambda_k z' - w_k x*',   lower bound: dL/dlb_j = w,   upper: dL/dub_j = -w,
// and zero for everything outside W.  |W| = nv: z = 0 exactly and N' w = gsol is a square system, solved on the
// normals themselves (Cramer's rule, GiSmall::solve_square) instead of on N D^-1 N', which squares their condition.
//
// Two conventions.  A variable pinned by lb == ub sits in W as ONE equality, the one solve_general pre-loads under
// the id of the lower bound: its w is reported as dL/dlb_j and dL/dub_j is zero.  An equality row may sit in W with
// its orientation reversed (the method turns an equality so that it reads n.x >= b and is violated): the slot then
// holds (-a_k, -b_k), and w and lambda of the slot change sign on their way to the row's gradient.
//
// Like gi_small.hpp the file compiles for the host (one lane per QP): tests/host_qp_vjp_driver.cpp runs this code on
// the CPU.  No loop indexes a register array by a run-time value: every pick is a select over the NV slots.
#pragma once
#include "gi_small.hpp"

namespace asif {

template <int NV>
struct QpAdjoint {
	double w[NV]; // per slot of the working set; zero for an empty slot
	double z[NV];
};

// The adjoint system for one problem.  Hd must be positive (the caller has checked it); the normal of an empty slot
// is zero, as GiWorkingSet promises.
template <int NV>
ASIF_HD void qp_adjoint_solve(const double (&Hd)[NV], const GiWorkingSet<NV> &ws, const double (&gsol)[NV], QpAdjoint<NV> &adj)
{
	static_assert(NV == 2 || NV == 3, "closed-form adjoint: two or three variables");
	double Pinv[NV];
#pragma unroll
	for (int j = 0; j < NV; j++) Pinv[j] = 1.0 / (2.0 * Hd[j]);
	bool full = true;
	double M[NV][NV], Mi[NV], r[NV];
#pragma unroll
	for (int s = 0; s < NV; s++) {
		const bool vs = ws.id[s] >= 0;
		full = full & vs;
		double d = 0.0;
#pragma unroll
		for (int j = 0; j < NV; j++) d += ws.nrm[s][j] * gsol[j] * Pinv[j];
		r[s] = vs ? d : 0.0;
#pragma unroll
		for (int t = 0; t <= s; t++) {
			double m = 0.0;
#pragma unroll
			for (int j = 0; j < NV; j++) m += ws.nrm[s][j] * ws.nrm[t][j] * Pinv[j];
			M[s][t] = (vs & (ws.id[t] >= 0)) ? m : (s == t ? 1.0 : 0.0);
		}
	}
	(void)ldl_factor<NV>(M, Mi); // W is linearly independent: the method only adds a normal outside the span of W
	ldl_solve<NV>(M, Mi, r);
	double rs[NV];
	(void)GiSmall<NV, 1, 1>::solve_square(ws.nrm, gsol, rs); // meaningful for a full W only
#pragma unroll
	for (int s = 0; s < NV; s++) adj.w[s] = full ? rs[s] : r[s];
#pragma unroll
	for (int j = 0; j < NV; j++) {
		double t = gsol[j];
#pragma unroll
		for (int s = 0; s < NV; s++) t -= ws.nrm[s][j] * adj.w[s];
		adj.z[j] = full ? 0.0 : t * Pinv[j];
	}
}

// dL/db_r and dL/dA_r = lambda_r z' - w_r x*' for general row r with coefficients a: zero unless r sits in W; signs
// follow the orientation the slot holds the row in.  ok: the instance is solved (selects: what an unsolved instance
// holds may be non-finite).
template <int NV>
ASIF_HD void qp_adjoint_row(const GiWorkingSet<NV> &ws, const QpAdjoint<NV> &adj, bool ok, int r, const double (&a)[NV],
                            const double (&x)[NV], double &gb, double (&gA)[NV])
{
	double wr = 0.0, lr = 0.0;
	bool in = false;
#pragma unroll
	for (int s = 0; s < NV; s++) {
		double dot = 0.0;
#pragma unroll
		for (int j = 0; j < NV; j++) dot += ws.nrm[s][j] * a[j];
		const bool mine = ws.id[s] == r;
		const double sg = dot < 0.0 ? -1.0 : 1.0;
		wr = mine ? sg * adj.w[s] : wr;
		lr = mine ? sg * ws.lam[s] : lr;
		in = in | mine;
	}
	in = in & ok;
	gb = in ? wr : 0.0;
#pragma unroll
	for (int j = 0; j < NV; j++) gA[j] = in ? lr * adj.z[j] - wr * x[j] : 0.0;
}

// dL/dlb_j and dL/dub_j
template <int NV>
ASIF_HD void qp_adjoint_bounds(const GiWorkingSet<NV> &ws, const QpAdjoint<NV> &adj, int j, double &glb, double &gub)
{
	glb = 0.0;
	gub = 0.0;
#pragma unroll
	for (int s = 0; s < NV; s++) {
		glb = ws.id[s] == GiSmall<NV, 1, 1>::kIdLb + j ? adj.w[s] : glb;
		gub = ws.id[s] == GiSmall<NV, 1, 1>::kIdUb + j ? 0.0 - adj.w[s] : gub;
	}
}

// What the kernel and the host driver do around the solve, in one place.
//
// solve_general leaves a wave together when one of its problems has a cost without curvature, and its loop runs
// until every lane of the wave is done: a problem the method cannot take -- non-finite data, some Hd_j <= 0 -- is
// therefore replaced by an inert one before the solve (selects; its verdict is fixed afterwards), so that what a
// solved instance computes never depends on the instances next to it.
template <int NV, int RPL, int G>
ASIF_HD int qp_vjp_solve(QpLaneData<NV, RPL> &qp, int g, double (&x)[NV], GiWorkingSet<NV> &ws)
{
	const bool nonfinite = qp_data_nonfinite<NV, RPL, G>(qp.Hd, qp.c, qp.lb, qp.ub, qp.A, qp.b);
	bool convex = true;
#pragma unroll
	for (int j = 0; j < NV; j++) convex = convex & (qp.Hd[j] > 0.0);
	const bool inert = nonfinite | !convex;
#pragma unroll
	for (int j = 0; j < NV; j++) {
		qp.Hd[j] = inert ? 1.0 : qp.Hd[j];
		qp.c[j] = inert ? 0.0 : qp.c[j];
		qp.lb[j] = inert ? -1.0 : qp.lb[j];
		qp.ub[j] = inert ? 1.0 : qp.ub[j];
	}
#pragma unroll
	for (int k = 0; k < RPL; k++) {
#pragma unroll
		for (int j = 0; j < NV; j++) qp.A[k][j] = inert ? 0.0 : qp.A[k][j];
		qp.b[k] = inert ? -1e20 : qp.b[k];
		qp.eq[k] = inert ? false : qp.eq[k];
	}
	int steps;
	const int verdict = GiSmall<NV, RPL, G>::template solve_general<true>(qp, g, 8 * NV + 4, x, steps, &ws);
	// rc of the entry: 1 solved, -1 infeasible or non-finite data, 0 undecided (no curvature, step budget, ambiguity)
	const int rc = verdict == kGiOptimal ? 1 : (verdict == kGiUndecided ? 0 : -1);
	return nonfinite ? -1 : (convex ? rc : 0);
}

} // namespace asif
