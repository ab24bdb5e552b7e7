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
// Models: DoubleIntegrator and CartPendulum (one input, functors that do not read DevOptions); the launchers at the end
// dispatch on the handle's model.  A model with kJointFunctors (CartPendulum: one sine / cosine pair per step) is called
// through its joint forms, model_step_functors / model_adjoint_functors of rollout_vjp_step.hpp.
// The kernel templates themselves are in rollout_policy_kernels.hpp (k_rollout_plant.hip instantiates them a second time,
// with the plant stepped by RK4); this file instantiates them for the models as they are and holds the four launchers.
#include "rollout_policy_kernels.hpp"

namespace asif {

template <class M, bool PARAMS>
static int launch_forward(const DevOptions &o, const ParamRolloutArgs &a, hipStream_t stream)
{
	if (a.p.B <= 0 || a.p.T <= 0) return 0;
	const dim3 grid(grid_for(a.p.B, 1, 256)), block(256);
	const RolloutVjpOpts<M::NU> e = rollout_class_opts<M>(o);
	if (a.p.v) hipLaunchKernelGGL((rollout_policy_kernel<M, true, PARAMS>), grid, block, 0, stream, e, a);
	else hipLaunchKernelGGL((rollout_policy_kernel<M, false, PARAMS>), grid, block, 0, stream, e, a);
	return (int)hipGetLastError();
}

template <class M, bool PARAMS, bool WANTP>
static int launch_backward(const DevOptions &o, const ParamRolloutVjpArgs &a, hipStream_t stream)
{
	if (a.p.B <= 0) return 0;
	hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, PARAMS, WANTP>), dim3(grid_for(a.p.B, 1, 256)), dim3(256), 0, stream,
	                   rollout_class_opts<M>(o), a);
	return (int)hipGetLastError();
}

int launch_rollout_policy_explicit(int model, const DevOptions &o, const PolicyRolloutArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) {
		return launch_forward<decltype(m), false>(o, ParamRolloutArgs{a, nullptr, nullptr, nullptr}, stream);
	});
}

// T == 0 runs the kernel too: it writes the identity (gx0 = gxT, guact0 = guactT or 0, gk = 0, gK = 0, nskip = 0, no gv)
int launch_rollout_policy_vjp_explicit(int model, const DevOptions &o, const PolicyRolloutVjpArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) {
		return launch_backward<decltype(m), false, false>(
			o, ParamRolloutVjpArgs{a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, stream);
	});
}

// the PARAMS kernels also where all three parameters are absent
int launch_rollout_params_explicit(int model, const DevOptions &o, const ParamRolloutArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) { return launch_forward<decltype(m), true>(o, a, stream); });
}

// T == 0: the identity of launch_rollout_policy_vjp_explicit, and galpha = glb = gub = 0
int launch_rollout_params_vjp_explicit(int model, const DevOptions &o, const ParamRolloutVjpArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) {
		if (a.galpha || a.glb || a.gub) return launch_backward<decltype(m), true, true>(o, a, stream);
		return launch_backward<decltype(m), true, false>(o, a, stream);
	});
}

} // namespace asif
