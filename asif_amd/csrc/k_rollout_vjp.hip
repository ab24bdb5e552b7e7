// k_rollout_vjp.hip -- the fused explicit rollout (k_explicit.hip: explicit_rollout_kernel) backwards: given the
// gradient of a scalar loss with respect to x_T, the last applied input and the logged states and inputs, the gradient
// with respect to x_0, uDes and the input handed in, for a batch, in one launch.
//
// One sweep t = T-1 ... 0 per instance over the logs the forward pass wrote; the step itself -- the plant's Euler step
// backwards, the forward solve repeated on the logged state, the filter's adjoint at its working set, the model's
// second derivatives -- is rollout_vjp_step.hpp.  lambda = dL/dx, mu = dL/du and the sum for dL/duDes stay in registers
// for the whole sweep; one instance per lane, SoA, every load and store a coalesced line, no LDS, no ADMM / finish code.
// HBM traffic per step and instance: 8 nx + 8 nu + 4 bytes of logs, and 8 (nx + nu) of their gradients where given.
// The loads of step t-1 depend on nothing step t computes: they are issued before step t's solve.
#include <cstdint>
#include "launchers.hpp"
#include "rollout_vjp_step.hpp"

namespace asif {

template <class M>
struct StepLogs {
	double x[M::NX], u[M::NU], gx[M::NX], gu[M::NU];
	int rc;
};

template <class M>
__device__ __forceinline__ void load_step(const RolloutVjpArgs &a, int t, int64_t i, StepLogs<M> &L)
{
	constexpr int NX = M::NX, NU = M::NU;
#pragma unroll
	for (int k = 0; k < NX; k++) {
		const int64_t at = ((int64_t)t * NX + k) * a.ld + i;
		L.x[k] = a.xlog[at];
		L.gx[k] = a.gxlog ? a.gxlog[at] : 0.0; // wave-uniform
	}
#pragma unroll
	for (int j = 0; j < NU; j++) {
		const int64_t at = ((int64_t)t * NU + j) * a.ld + i;
		L.u[j] = a.ulog[at];
		L.gu[j] = a.gulog ? a.gulog[at] : 0.0;
	}
	L.rc = a.rclog[(int64_t)t * a.ld + i];
}

template <class M>
__global__ __launch_bounds__(256) void rollout_vjp_kernel(RolloutVjpOpts<M::NU> e, RolloutVjpArgs a)
{
	static_assert(M::kIgnoresOptions, "the model's functors must not read DevOptions: only the class's fields are passed");
	constexpr int NX = M::NX, NU = M::NU;
	const DevOptions o = {};
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the wave votes of the solve; it never stores

	double uDes[NU];
	RolloutAdjoint<M> s;
#pragma unroll
	for (int k = 0; k < NX; k++) s.lam[k] = a.gxT[k * a.ld + i];
#pragma unroll
	for (int j = 0; j < NU; j++) {
		uDes[j] = a.udes[j * a.ld + i];
		s.mu[j] = a.guactT ? a.guactT[j * a.ld + i] : 0.0;
		s.gudes[j] = 0.0;
	}
	s.nskip = 0;

	StepLogs<M> cur = {}, nxt = {};
	if (a.T > 0) load_step<M>(a, a.T - 1, i, cur);
#pragma unroll 1
	for (int t = a.T - 1; t >= 0; t--) { // wave-uniform trip count
		if (t > 0) load_step<M>(a, t - 1, i, nxt); // in flight behind this step's solve
		rollout_vjp_step<M>(o, e, a.dt, cur.x, cur.u, uDes, cur.rc, cur.gx, cur.gu, s);
		cur = nxt;
	}
	if (!live) return;
#pragma unroll
	for (int k = 0; k < NX; k++) a.gx0[k * a.ld + i] = s.lam[k];
#pragma unroll
	for (int j = 0; j < NU; j++) {
		a.gudes[j * a.ld + i] = s.gudes[j];
		a.guact0[j * a.ld + i] = s.mu[j];
	}
	a.nskip[i] = s.nskip;
}

// T == 0 runs the kernel too: it writes the identity (gx0 = gxT, guact0 = guactT or 0, gudes = 0, nskip = 0)
int launch_rollout_vjp_explicit_di(const DevOptions &o, const RolloutVjpArgs &a, hipStream_t stream)
{
	using M = DoubleIntegrator;
	if (a.B <= 0) return 0;
	const int block = 256;
	hipLaunchKernelGGL((rollout_vjp_kernel<M>), dim3(grid_for(a.B, 1, block)), dim3(block), 0, stream,
	                   rollout_class_opts<M>(o), a);
	return (int)hipGetLastError();
}

} // namespace asif
