// k_rollout_policy.hip -- the fused explicit rollout (k_explicit.hip: explicit_rollout_kernel, light instantiation) with
// the desired input coming from an affine policy evaluated inside the loop, optionally with the filter's own parameters
// per instance, and its adjoint:
//     uDes_t = k + K x_t + v_t;   (ok_t, u*_t) = filter(x_t, uDes_t; alpha_i, lb_i, ub_i);   u_t = ok_t ? u*_t : u_{t-1};
//     x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
// K (feedback gains, per instance) and v (a planned input sequence) are each optional; without both the forward kernel
// computes what explicit_rollout_kernel<M, true> computes with udes = k, bit for bit, and the backward kernel what
// rollout_vjp_kernel computes, with gk in the place of gudes.
// Two uses, one source.  The policy entries (PARAMS = false) filter with the handle's options, which stay in scalar
// registers.  The params entries (PARAMS = true) take alpha (the barrier gain: DevOptions::relaxLb), lb and ub per
// instance, each optional: an absent one is the handle's value in every lane, and without all three they compute what the
// policy entries compute, bit for bit.
//
// Forward: one instance per lane, 256-thread workgroups, x / uAct / K / k (and the three parameters) in registers for the
// whole rollout, the dual active-set stage decides every step (no ADMM / finish code).  v_{t+1} depends on nothing step t
// computes: it is loaded before step t's solve and waited for in front of step t's stores.  The step's QP is
// explicit_step_qp (rollout_vjp_step.hpp); the plant step restates explicit_rollout_kernel's.
// Backward: rollout_vjp_kernel's structure around rollout_params_step.hpp; lambda, mu, gk, gK (and galpha, glb, gub) in
// registers, the logs, their gradients and v of step t-1 loaded behind step t's solve, gv[t] = d_t stored per step where
// the caller asked for it.  WANTP (one of the three parameter gradients is asked for) is a template argument: without it
// the step hands nothing out and the loop is the policy entry's.
// HBM traffic per step and instance.  Forward: 8 nu read (v), 8 nx + 8 nu + 4 written (logs).  Backward: 8 nx + 8 nu + 4
// of logs and 8 nu of v read, 8 (nx + nu) of log gradients where given, 8 nu written (gv) where asked for.  Per instance
// and LAUNCH on top of that: 8 bytes read per parameter given, 8 written per parameter gradient asked for.
// SoA, every load and store a coalesced line; no LDS, no scratch, no register array indexed by a run-time value.  Lanes
// beyond B repeat instance B-1 for the solver's votes and never store.
// Models: DoubleIntegrator and CartPendulum (with_rollout_model, launchers.hpp).  A model with kJointFunctors
// (CartPendulum: one sine / cosine pair per step) is called through its joint forms, model_step_functors /
// model_adjoint_functors of rollout_vjp_step.hpp.
// The kernel templates and the two launch templates (grid, HASV, WANTP) are in rollout_policy_kernels.hpp.  This file
// instantiates them for the models as they are, PARAMS false and true, and holds the two launchers every entry goes
// through: the policy entries (params = false), the params entries and the plant entries under Euler (params = true) run
// this file's kernels; the plant entries under RK4 are handed to k_rollout_plant.hip, which instantiates the templates a
// second time on WithRk4<model>.
#include "rollout_policy_kernels.hpp"

namespace asif {

int launch_rollout_policy_explicit(int model, int integrator, bool params, const DevOptions &o, const ParamRolloutArgs &a,
                                   hipStream_t stream)
{
	if (integrator == ASIF_HIP_PLANT_RK4) return params ? launch_rk4(model, o, a, stream) : ASIF_HIP_EUNSUPPORTED;
	if (integrator != ASIF_HIP_PLANT_EULER) return ASIF_HIP_EINVAL;
	return with_rollout_model(model, [&](auto m) {
		using M = decltype(m);
		return params ? launch_forward<M, true>(o, a, stream) : launch_forward<M, false>(o, a, stream);
	});
}

int launch_rollout_policy_vjp_explicit(int model, int integrator, bool params, const DevOptions &o,
                                       const ParamRolloutVjpArgs &a, hipStream_t stream)
{
	if (integrator == ASIF_HIP_PLANT_RK4) return params ? launch_rk4(model, o, a, stream) : ASIF_HIP_EUNSUPPORTED;
	if (integrator != ASIF_HIP_PLANT_EULER) return ASIF_HIP_EINVAL;
	return with_rollout_model(model, [&](auto m) {
		using M = decltype(m);
		return params ? launch_backward<M, true>(o, a, stream) : launch_backward<M, false>(o, a, stream);
	});
}

} // namespace asif
