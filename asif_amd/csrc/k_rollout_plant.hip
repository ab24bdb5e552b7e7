// k_rollout_plant.hip -- the fused explicit rollout under an affine policy with the filter's parameters per instance
// (k_rollout_policy.hip, PARAMS) and its adjoint, with the plant's integrator chosen by the caller:
//     uDes_t = k + K x_t + v_t;   (ok_t, u*_t) = filter(x_t, uDes_t; alpha_i, lb_i, ub_i);   u_t = ok_t ? u*_t : u_{t-1};
//     x_{t+1} = step(x_t, u_t, dt)     with u_t held over the control period
// Euler is k_rollout_policy.hip's own kernels, launched through its launchers: nothing is compiled for it here.  RK4
// (plant_step.hpp) is compiled here, from the same kernel templates (rollout_policy_kernels.hpp) on WithRk4<model>, PARAMS
// always: the loop, the lane rule, the prefetches behind the solve and the waits in front of the stores are theirs.
// Forward: three more evaluations of f and g per step (on the pendulum one sine / cosine pair each), between the step's
// stores and the next step's policy; k1 is formed from the f and g the filter's rows were.  Backward: the stage states
// are recomputed from the logged (x_t, u_t) and the plant's adjoint runs through them before the step's QP is
// assembled, so no stage value is live across the solve.  HBM traffic is k_rollout_policy.hip's: no further log.
// The filter is evaluated at x_t only: the barrier condition holds at the sample instants, not between them.
#include "rollout_policy_kernels.hpp"

namespace asif {

int launch_rollout_plant_explicit(int model, int integrator, const DevOptions &o, const ParamRolloutArgs &a,
                                  hipStream_t stream)
{
	if (integrator == ASIF_HIP_PLANT_EULER) return launch_rollout_params_explicit(model, o, a, stream);
	if (integrator != ASIF_HIP_PLANT_RK4) return ASIF_HIP_EINVAL;
	return with_rollout_model(model, [&](auto m) {
		using M = WithRk4<decltype(m)>;
		if (a.p.B <= 0 || a.p.T <= 0) return 0;
		const dim3 grid(grid_for(a.p.B, 1, 256)), block(256);
		const RolloutVjpOpts<M::NU> e = rollout_class_opts<M>(o);
		if (a.p.v) hipLaunchKernelGGL((rollout_policy_kernel<M, true, true>), grid, block, 0, stream, e, a);
		else hipLaunchKernelGGL((rollout_policy_kernel<M, false, true>), grid, block, 0, stream, e, a);
		return (int)hipGetLastError();
	});
}

// T == 0 runs the kernel too: the identity of launch_rollout_params_vjp_explicit
int launch_rollout_plant_vjp_explicit(int model, int integrator, const DevOptions &o, const ParamRolloutVjpArgs &a,
                                      hipStream_t stream)
{
	if (integrator == ASIF_HIP_PLANT_EULER) return launch_rollout_params_vjp_explicit(model, o, a, stream);
	if (integrator != ASIF_HIP_PLANT_RK4) return ASIF_HIP_EINVAL;
	return with_rollout_model(model, [&](auto m) {
		using M = WithRk4<decltype(m)>;
		if (a.p.B <= 0) return 0;
		const dim3 grid(grid_for(a.p.B, 1, 256)), block(256);
		const RolloutVjpOpts<M::NU> e = rollout_class_opts<M>(o);
		if (a.galpha || a.glb || a.gub) hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, true, true>), grid, block, 0, stream, e, a);
		else hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, true, false>), grid, block, 0, stream, e, a);
		return (int)hipGetLastError();
	});
}

} // namespace asif
