// rollout_params_step.hpp -- the fused explicit rollout under an affine policy with the filter's own parameters per
// instance: the barrier gain alpha_i (DevOptions::relaxLb, the value the relaxation variable is pinned to) and the input
// box lb_i, ub_i.  Per instance and in registers: the rule for a usable gain, and one step of the adjoint.
//
// Forward step t (k_rollout_params.hip: rollout_params_kernel): rollout_policy_step.hpp's, with the QP formed from the
// instance's values -- rows Lgh u + alpha_i h >= -Lfh, box lb_i <= u <= ub_i, the final clamp to that box.
//
// Backward step: rollout_policy_vjp_step unchanged, handed a RolloutVjpOpts filled from the instance's values (so its
// state gradient uses alpha_i where it reads e.relaxLb), and in front of it params_step_grads, which repeats the step's
// solve for the working set W and the multiplier w of the adjoint system and adds, on a solved step,
//     galpha += -h_r w      W = safety row r       (u* = (-Lfh_r - alpha h_r) / Lgh_r,  w = mu / Lgh_r)
//     glb_j  +=  w          W = lower bound of j   (normal +1: w = mu)
//     gub_j  += -w          W = upper bound of j   (normal -1: -w = mu)
// A failed step and a free step add nothing.  Kinks on the side the forward pass took, as the step it wraps.  With one
// input the solve is closed form and straight-line: repeated next to the wrapped step's own, the compiler merges the two.
//
// Compiles for the host like the files it wraps (tests/host_rollout_params_driver.cpp).
#pragma once
#include "rollout_policy_step.hpp"

namespace asif {

// A gain handed in per instance must be a positive finite number: zero or a negative gain is no class-K function, and the
// instance's every step then fails (rc -1) like a step on non-finite data.  The handle's own value is taken as it is.
ASIF_HD bool param_gain_usable(double alpha) { return alpha > 0.0 && alpha < __builtin_huge_val(); }

template <class M>
struct ParamAdjoint { // what the parameter sweep carries from step to step
	PolicyAdjoint<M> p;
	double galpha, glb[M::NU], gub[M::NU];
};

// The three sums of one step.  lam, mu: the sweep's values BEFORE the step; uDes: policy_udes on x.
template <class M, class O>
ASIF_HD void params_step_grads(const O &o, const RolloutVjpOpts<M::NU> &e, double dt, const double (&x)[M::NX],
                               const double (&uDes)[M::NU], int rc, const double (&gul)[M::NU],
                               const double (&lam)[M::NX], const double (&mu)[M::NU], double &galpha,
                               double (&glb)[M::NU], double (&gub)[M::NU])
{
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS, NV = NU + 1, NC = NP;
	static_assert(NU == 1, "one input: W holds one constraint and w = mu / its normal");
	double h[NP], Dh[NP * NX], f[NX], gm[NX * NU];
	M::safetySet(o, x, h, Dh);
	M::dynamics(o, x, f, gm);
	double gbar[NU]; // mu as the step's filter sees it
#pragma unroll
	for (int j = 0; j < NU; j++) {
		double t = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) t += gm[k + j * NX] * lam[k];
		gbar[j] = mu[j] + (gul[j] + dt * t);
	}
	// the rows, as rollout_vjp_step assembles them
	const int nkeep = e.npKeep;
	bool kept[NP];
#pragma unroll
	for (int r = 0; r < NP; r++) kept[r] = true;
	if (nkeep < NP) { // the same for every instance of a launch
#pragma unroll
		for (int r = 0; r < NP; r++) {
			int p = 0;
#pragma unroll
			for (int q = 0; q < NP; q++) p += (h[q] < h[r] || (h[q] == h[r] && q < r)) ? 1 : 0;
			kept[r] = p < nkeep;
		}
	}
	QpLaneData<NV, NC> qp;
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
#pragma unroll
	for (int r = 0; r < NC; r++) {
		double a = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) a += Dh[r + k * NP] * f[k];
#pragma unroll
		for (int j = 0; j < NU; j++) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) t += Dh[r + k * NP] * gm[k + j * NX];
			qp.A[r][j] = kept[r] ? t : 0.0;
		}
		qp.A[r][NU] = kept[r] ? h[r] : 0.0;
		qp.b[r] = kept[r] ? -a : -1e20;
		qp.eq[r] = false;
	}
	double sol[NV];
	int steps;
	GiWorkingSet<NU> ws;
	const int verdict = GiSmall<NV, NC, 1>::template solve_with_pinned_ws<NU>(qp, 0, 8 * NV + 4, sol, steps, ws);
	const bool use = (rc == 1) & (verdict == kGiOptimal);
	const int id = ws.id[0];
	const double w = id >= 0 ? gbar[0] / ws.nrm[0][0] : 0.0;
	// selects: a step that is not used may hold non-finite data
	double ga = 0.0;
#pragma unroll
	for (int r = 0; r < NP; r++) ga = (id == r) ? 0.0 - h[r] * w : ga;
	galpha += use ? ga : 0.0;
	glb[0] += (use & (id == GiSmall<NU, NC, 1>::kIdLb)) ? w : 0.0;
	gub[0] += (use & (id == GiSmall<NU, NC, 1>::kIdUb)) ? 0.0 - w : 0.0;
}

// wantP: one of galpha, glb, gub is asked for (the same for every instance of a launch)
template <class M, class O>
ASIF_HD void rollout_params_vjp_step(const O &o, const RolloutVjpOpts<M::NU> &e, double dt, const double (&x)[M::NX],
                                     const double (&ut)[M::NU], const double (&k)[M::NU],
                                     const double (&K)[M::NU * M::NX], bool hasK, const double (&v)[M::NU], bool hasV,
                                     int rc, const double (&gxl)[M::NX], const double (&gul)[M::NU], bool wantP,
                                     ParamAdjoint<M> &q)
{
	if (wantP) {
		double uDes[M::NU];
		policy_udes<M::NX, M::NU>(k, K, hasK, x, v, hasV, uDes);
		params_step_grads<M>(o, e, dt, x, uDes, rc, gul, q.p.s.lam, q.p.s.mu, q.galpha, q.glb, q.gub);
	}
	rollout_policy_vjp_step<M>(o, e, dt, x, ut, k, K, hasK, v, hasV, rc, gxl, gul, q.p);
}

} // namespace asif
