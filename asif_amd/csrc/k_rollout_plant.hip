// k_rollout_plant.hip -- the fused explicit rollout under an affine policy with the filter's parameters per instance
// (k_rollout_policy.hip, PARAMS) and its adjoint, with the plant's integrator chosen by the caller:
//     uDes_t = k + K x_t + v_t;   (ok_t, u*_t) = filter(x_t, uDes_t; alpha_i, lb_i, ub_i);   u_t = ok_t ? u*_t : u_{t-1};
//     x_{t+1} = step(x_t, u_t, dt)     with u_t held over the control period
// Euler is k_rollout_policy.hip's own kernels, launched by its two launchers: nothing is compiled for it here.  RK4
// (plant_step.hpp) is compiled here and nowhere else, from the same kernel and launch templates
// (rollout_policy_kernels.hpp) on WithRk4<model>, PARAMS always: the loop, the lane rule, the prefetches behind the solve
// and the waits in front of the stores are theirs.  The two launchers of k_rollout_policy.hip hand the plant entries'
// RK4 calls to launch_rk4 below.
// Forward: three more evaluations of f and g per step (on the pendulum one sine / cosine pair each), between the step's
// stores and the next step's policy; k1 is formed from the f and g the filter's rows were.  Backward: the stage states
// are recomputed from the logged (x_t, u_t) and the plant's adjoint runs through them before the step's QP is
// assembled, so no stage value is live across the solve.  HBM traffic is k_rollout_policy.hip's: no further log.
// The filter is evaluated at x_t only: the barrier condition holds at the sample instants, not between them.
#include "rollout_policy_kernels.hpp"

namespace asif {

int launch_rk4(int model, const DevOptions &o, const ParamRolloutArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) { return launch_forward<WithRk4<decltype(m)>, true>(o, a, stream); });
}

int launch_rk4(int model, const DevOptions &o, const ParamRolloutVjpArgs &a, hipStream_t stream)
{
	return with_rollout_model(model, [&](auto m) { return launch_backward<WithRk4<decltype(m)>, true>(o, a, stream); });
}

} // namespace asif
