// rollout_vjp_step.hpp -- one step of the adjoint of the fused explicit rollout (k_explicit.hip: explicit_rollout_kernel),
// for one instance, in registers.
//
// The forward step on the state x_t the filter saw, with u_{t-1} the input applied before it:
//     (ok_t, u*_t) = filter(x_t, uDes);   u_t = ok_t ? u*_t : u_{t-1};   x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
// With lambda = dL/dx_{t+1} and mu = dL/du_t collected from the later steps, gxl / gul the loss's own gradient on the
// logged x_t / u_t, the step backwards is
//     mu      += gul + dt g(x_t)' lambda
//     lambda'  = lambda + dt (Df(x_t) + sum_j u_t,j Dg_j(x_t))' lambda + gxl
//     rc_t == 1:  the filter's adjoint at gbar = mu (k_explicit_vjp.hip:1-12): the forward solve is repeated on x_t,
//                 W is the working set it ends with, 2 z + G_W' w = gbar, G_W z = 0, and
//                     gudes   += 2 z
//                     lambda' += Dh' gh + (dLfh/dx)' glfh + (dLgh/dx)' glgh,   mu = 0
//                 with glfh_k = -w_k, glgh_k = lambda_k z' - w_k u*', gh_k = -relaxLb w_k on the rows of W and
//                     dLfh_r/dx_m   = sum_k (D2h_r[k,m] f_k     + Dh_r[k] Df[k,m])
//                     dLgh_r,j/dx_m = sum_k (D2h_r[k,m] g_{k,j} + Dh_r[k] Dg_j[k,m])
//     otherwise:  mu passes on unchanged (the step kept u_{t-1})
// Kinks are taken on the side the forward pass took: the branch of the model's safety set, the row order under
// npSSmax, a constraint met with equality but outside W, the clamp.
//
// out, where given, receives the step's verdict, W, w and h: the filter's parameters enter the QP only through the rows'
// h column and the box, so their gradients are sums over these (rollout_params_step.hpp) and need no solve of their own.
//
// rc is the caller's record of what the forward pass decided.  rc == 1 next to a solve of this file that does not end
// optimal (not possible on the same code and the same bits) contributes nothing: mu = 0 and the step is counted.
//
// M supplies safetySet, dynamics, safetyHess and dynamicsJac (models.hpp) or, where it declares kJointFunctors, their joint
// forms (model_adjoint_functors below); O is whatever those functors take as their first argument.  Like gi_small.hpp the file compiles for the host: tests/host_rollout_vjp_driver.cpp runs it on the
// CPU with a plain C++ copy of the model's functors.  No loop indexes a register array by a run-time value.
#pragma once
#include <type_traits>
#include "gi_small.hpp"
#include "plant_step.hpp"

namespace asif {

template <int NU>
struct RolloutVjpOpts { // the fields of DevOptions the explicit class reads (see explicit_light_kernel)
	double lb[NU], ub[NU], relaxCost, relaxLb;
	int npKeep;
};

// o: DevOptions (a template argument only because this file compiles for the host without models.hpp)
template <class M, class DO>
inline RolloutVjpOpts<M::NU> rollout_class_opts(const DO &o)
{
	RolloutVjpOpts<M::NU> e;
	for (int j = 0; j < M::NU; j++) {
		e.lb[j] = o.lb[j];
		e.ub[j] = o.ub[j];
	}
	e.relaxCost = o.relaxCost;
	e.relaxLb = o.relaxLb;
	e.npKeep = o.npKeep < M::NPSS ? o.npKeep : M::NPSS;
	return e;
}

// The QP of the explicit class at one state, from the model's h, Dh, f, g there: the one statement of it for the fused
// rollouts under a policy and for every adjoint step (explicit_rollout_kernel in k_explicit.hip keeps a copy of its own).
//     min |u - uDes|^2 + relaxCost (d - relaxLb)^2   s.t.  Lgh_r u + h_r d >= -Lfh_r,  lb <= u <= ub,  d = relaxLb
// with Lfh = Dh f, Lgh = Dh g and the relaxation variable d, the last one, pinned by its bounds.  npKeep < NP (npSSmax <
// npSS): only the rows of the npKeep smallest h count, ties going to the lower index; the others are zero with
// b = -1e20, inert.
template <int NX, int NU, int NP>
ASIF_HD void explicit_step_qp(const double (&h)[NP], const double (&Dh)[NP * NX], const double (&f)[NX],
                              const double (&gm)[NX * NU], const double (&uDes)[NU], const RolloutVjpOpts<NU> &e,
                              QpLaneData<NU + 1, NP> &qp)
{
#pragma unroll
	for (int r = 0; r < NP; r++) {
		double s = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) s += Dh[r + k * NP] * f[k];
#pragma unroll
		for (int j = 0; j < NU; j++) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) t += Dh[r + k * NP] * gm[k + j * NX];
			qp.A[r][j] = t;
		}
		qp.A[r][NU] = h[r];
		qp.b[r] = -s;
		qp.eq[r] = false;
	}
	if (e.npKeep < NP) { // the same for every instance of a launch
#pragma unroll
		for (int r = 0; r < NP; r++) {
			int p = 0;
#pragma unroll
			for (int q = 0; q < NP; q++) p += (h[q] < h[r] || (h[q] == h[r] && q < r)) ? 1 : 0;
			const bool kept = p < e.npKeep;
#pragma unroll
			for (int j = 0; j < NU + 1; j++) qp.A[r][j] = kept ? qp.A[r][j] : 0.0;
			qp.b[r] = kept ? qp.b[r] : -1e20;
		}
	}
#pragma unroll
	for (int j = 0; j < NU; j++) {
		qp.Hd[j] = 1.0;
		qp.c[j] = -2.0 * uDes[j];
		qp.lb[j] = e.lb[j];
		qp.ub[j] = e.ub[j];
	}
	qp.Hd[NU] = e.relaxCost;
	qp.c[NU] = -2.0 * e.relaxCost * e.relaxLb;
	qp.lb[NU] = e.relaxLb;
	qp.ub[NU] = e.relaxLb;
}

// A model with kJointFunctors (plant_step.hpp: joint_functors) supplies stepFunctors (safetySet + dynamics) and
// adjointFunctors (all four) -- the same values as the four functors one by one, evaluated together.  Every other model is
// called functor by functor, as before.
template <class M, class O>
ASIF_HD void model_step_functors(const O &o, const double (&x)[M::NX], double (&h)[M::NPSS], double (&Dh)[M::NPSS * M::NX],
                                 double (&f)[M::NX], double (&gm)[M::NX * M::NU])
{
	if constexpr (joint_functors<M>::value) {
		M::stepFunctors(o, x, h, Dh, f, gm);
	} else {
		M::safetySet(o, x, h, Dh);
		M::dynamics(o, x, f, gm);
	}
}

template <class M, class O>
ASIF_HD void model_adjoint_functors(const O &o, const double (&x)[M::NX], double (&h)[M::NPSS],
                                    double (&Dh)[M::NPSS * M::NX], double (&f)[M::NX], double (&gm)[M::NX * M::NU],
                                    double (&D2h)[M::NPSS * M::NX * M::NX], double (&Df)[M::NX * M::NX],
                                    double (&Dg)[M::NX * M::NX * M::NU])
{
	if constexpr (joint_functors<M>::value) {
		M::adjointFunctors(o, x, h, Dh, f, gm, D2h, Df, Dg);
	} else {
		M::safetySet(o, x, h, Dh);
		M::dynamics(o, x, f, gm);
		M::safetyHess(o, x, D2h);
		M::dynamicsJac(o, x, Df, Dg);
	}
}

template <class M>
struct RolloutAdjoint { // what the sweep carries from step to step
	double lam[M::NX], mu[M::NU], gudes[M::NU];
	int nskip;
};

template <class M>
struct StepWorkingSet { // what a step knows of its filter call, for a caller that differentiates the filter's parameters
	bool use;           // rc == 1 and the repeated solve ended optimal
	int id[M::NU];      // W, ids as GiWorkingSet's
	double w[M::NU], h[M::NPSS]; // the multiplier of the adjoint system per slot of W; the safety functions at x
};

// PLANT: the plant's integrator (plant_step.hpp), Euler unless the caller says otherwise
template <class M, int PLANT = kPlantEuler, class O>
ASIF_HD void rollout_vjp_step(const O &o, const RolloutVjpOpts<M::NU> &e, double dt, const double (&x)[M::NX],
                              const double (&ut)[M::NU], const double (&uDes)[M::NU], int rc, const double (&gxl)[M::NX],
                              const double (&gul)[M::NU], RolloutAdjoint<M> &s, StepWorkingSet<M> *out = nullptr)
{
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS, NV = NU + 1, NC = NP;
	static_assert(NU == 1 || NU == 2, "closed-form adjoint: 1 x 1 or 2 x 2");
	double h[NP], Dh[NP * NX], f[NX], gm[NX * NU], D2h[NP * NX * NX], Df[NX * NX], Dg[NX * NX * NU];
	model_adjoint_functors<M>(o, x, h, Dh, f, gm, D2h, Df, Dg);

	// ---- 1. the plant's step backwards (plant_step.hpp)
	double lamn[NX];
	if constexpr (PLANT == kPlantEuler) {
#pragma unroll
		for (int j = 0; j < NU; j++) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) t += gm[k + j * NX] * s.lam[k];
			s.mu[j] += gul[j] + dt * t;
		}
#pragma unroll
		for (int m = 0; m < NX; m++) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) {
				double c = Df[k + m * NX];
#pragma unroll
				for (int j = 0; j < NU; j++) c += ut[j] * Dg[k + m * NX + j * NX * NX];
				t += c * s.lam[k];
			}
			lamn[m] = s.lam[m] + dt * t + gxl[m];
		}
	} else {
		plant_step_adjoint<M, PLANT>(o, dt, x, ut, f, gm, Df, Dg, s.lam, gxl, gul, s.mu, lamn);
	}

	// ---- 2. the step's QP
	QpLaneData<NV, NC> qp;
	explicit_step_qp<NX, NU, NP>(h, Dh, f, gm, uDes, e, qp);

	// ---- 3. the forward solve, and the working set it ends with
	double sol[NV];
	int steps;
	GiWorkingSet<NU> ws;
	const int verdict = GiSmall<NV, NC, 1>::template solve_with_pinned_ws<NU>(qp, 0, 8 * NV + 4, sol, steps, ws);
	const bool solved = rc == 1, use = solved & (verdict == kGiOptimal);
	s.nskip += (solved & !use) ? 1 : 0;

	// ---- 4. the filter's adjoint at gbar = mu.  w[t] belongs to slot t; the normal of an empty slot is zero
	double u[NU], w[NU], z[NU];
#pragma unroll
	for (int j = 0; j < NU; j++) u[j] = fmin(fmax(sol[j], e.lb[j]), e.ub[j]); // inputSaturate, src/asif.cpp:343-352
	if constexpr (NU == 1) {
		const bool in = ws.id[0] >= 0;
		w[0] = in ? s.mu[0] / ws.nrm[0][0] : 0.0;
		z[0] = in ? 0.0 : 0.5 * s.mu[0];
	} else {
		const double(&n0)[2] = ws.nrm[0], (&n1)[2] = ws.nrm[1];
		const bool v0 = ws.id[0] >= 0, v1 = ws.id[1] >= 0, both = v0 & v1, one = v0 != v1;
		const double det = n0[0] * n1[1] - n1[0] * n0[1];
		const double nn[2] = {n0[0] + n1[0], n0[1] + n1[1]}; // the one normal when `one`
		const double mm = nn[0] * nn[0] + nn[1] * nn[1];
		const double w1d = (nn[0] * s.mu[0] + nn[1] * s.mu[1]) / (one ? mm : 1.0);
		const double idet = 1.0 / (both ? det : 1.0);
		w[0] = both ? (s.mu[0] * n1[1] - n1[0] * s.mu[1]) * idet : ((one & v0) ? w1d : 0.0);
		w[1] = both ? (n0[0] * s.mu[1] - s.mu[0] * n0[1]) * idet : ((one & v1) ? w1d : 0.0);
#pragma unroll
		for (int j = 0; j < 2; j++) z[j] = both ? 0.0 : 0.5 * (s.mu[j] - w[0] * n0[j] - w[1] * n1[j]);
	}
	if (out) { // known where the call is inlined: a caller that passes nothing pays nothing
		out->use = use;
#pragma unroll
		for (int t = 0; t < NU; t++) out->id[t] = ws.id[t], out->w[t] = w[t];
#pragma unroll
		for (int r = 0; r < NP; r++) out->h[r] = h[r];
	}
	// per safety function: the gradient of its row (zero outside W), then its share of dL/dx_t through h, Lfh and Lgh
	double add[NX];
#pragma unroll
	for (int m = 0; m < NX; m++) add[m] = 0.0;
#pragma unroll
	for (int r = 0; r < NP; r++) {
		double wr = 0.0, lr = 0.0;
#pragma unroll
		for (int t = 0; t < NU; t++) {
			const bool mine = ws.id[t] == r;
			wr = mine ? w[t] : wr;
			lr = mine ? ws.lam[t] : lr;
		}
		const double gh = 0.0 - e.relaxLb * wr, glfh = 0.0 - wr;
		double glgh[NU];
#pragma unroll
		for (int j = 0; j < NU; j++) glgh[j] = lr * z[j] - wr * u[j];
#pragma unroll
		for (int m = 0; m < NX; m++) {
			double dlfh = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) dlfh += D2h[r + NP * (k + NX * m)] * f[k] + Dh[r + k * NP] * Df[k + m * NX];
			double t = Dh[r + m * NP] * gh + dlfh * glfh;
#pragma unroll
			for (int j = 0; j < NU; j++) {
				double dlgh = 0.0;
#pragma unroll
				for (int k = 0; k < NX; k++)
					dlgh += D2h[r + NP * (k + NX * m)] * gm[k + j * NX] + Dh[r + k * NP] * Dg[k + m * NX + j * NX * NX];
				t += dlgh * glgh[j];
			}
			add[m] += t;
		}
	}
	// selects: a step that is not used may hold non-finite data
#pragma unroll
	for (int j = 0; j < NU; j++) {
		s.gudes[j] += use ? 2.0 * z[j] : 0.0;
		s.mu[j] = solved ? 0.0 : s.mu[j];
	}
#pragma unroll
	for (int m = 0; m < NX; m++) s.lam[m] = lamn[m] + (use ? add[m] : 0.0);
}

} // namespace asif
