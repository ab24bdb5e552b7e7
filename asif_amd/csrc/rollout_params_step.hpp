// rollout_params_step.hpp -- the fused explicit rollout under an affine policy with the filter's own parameters per
// instance: the barrier gain alpha_i (DevOptions::relaxLb, the value the relaxation variable is pinned to) and the input
// box lb_i, ub_i.  Per instance and in registers: the rule for a usable gain, and one step of the adjoint.
//
// Forward step t (k_rollout_policy.hip: rollout_policy_kernel with PARAMS): rollout_policy_step.hpp's, with the QP formed
// from the instance's values -- rows Lgh u + alpha_i h >= -Lfh, box lb_i <= u <= ub_i, the final clamp to that box.
//
// Backward step: rollout_policy_vjp_step, handed a RolloutVjpOpts filled from the instance's values (so its state
// gradient uses alpha_i where it reads e.relaxLb).  Where a parameter gradient is asked for, the step also hands out its
// working set W, the multiplier w of its adjoint system and h (StepWorkingSet), and params_step_grads adds, on a solved
// step,
//     galpha += -h_r w      W = safety row r       (u* = (-Lfh_r - alpha h_r) / Lgh_r,  w = mu / Lgh_r)
//     glb_j  +=  w          W = lower bound of j   (normal +1: w = mu)
//     gub_j  += -w          W = upper bound of j   (normal -1: -w = mu)
// A failed step and a free step add nothing.  Kinks on the side the forward pass took, as the step it wraps.
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

// The three sums of one step, from what the step handed out.
template <class M>
ASIF_HD void params_step_grads(const StepWorkingSet<M> &ws, double &galpha, double (&glb)[M::NU], double (&gub)[M::NU])
{
	constexpr int NU = M::NU, NP = M::NPSS;
	static_assert(NU == 1, "one input: W holds one constraint and w = mu / its normal");
	const int id = ws.id[0];
	const double w = ws.w[0];
	// selects: a step that is not used may hold non-finite data
	double ga = 0.0;
#pragma unroll
	for (int r = 0; r < NP; r++) ga = (id == r) ? 0.0 - ws.h[r] * w : ga;
	galpha += ws.use ? ga : 0.0;
	glb[0] += (ws.use & (id == GiSmall<NU, NP, 1>::kIdLb)) ? w : 0.0;
	gub[0] += (ws.use & (id == GiSmall<NU, NP, 1>::kIdUb)) ? 0.0 - w : 0.0;
}

// wantP: one of galpha, glb, gub is asked for (the same for every instance of a launch)
template <class M, int PLANT = kPlantEuler, class O>
ASIF_HD void rollout_params_vjp_step(const O &o, const RolloutVjpOpts<M::NU> &e, double dt, const double (&x)[M::NX],
                                     const double (&ut)[M::NU], const double (&k)[M::NU],
                                     const double (&K)[M::NU * M::NX], bool hasK, const double (&v)[M::NU], bool hasV,
                                     int rc, const double (&gxl)[M::NX], const double (&gul)[M::NU], bool wantP,
                                     ParamAdjoint<M> &q)
{
	StepWorkingSet<M> ws;
	rollout_policy_vjp_step<M, PLANT>(o, e, dt, x, ut, k, K, hasK, v, hasV, rc, gxl, gul, q.p, wantP ? &ws : nullptr);
	if (wantP) params_step_grads<M>(ws, q.galpha, q.glb, q.gub);
}

} // namespace asif
