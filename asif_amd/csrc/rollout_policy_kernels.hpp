// rollout_policy_kernels.hpp -- the kernels of the fused rollout under an affine policy and of its adjoint, one instance
// per lane, and their launches: what k_rollout_policy.hip describes.  Two translation units instantiate them:
// k_rollout_policy.hip for the models as they are (Euler: the policy and the params entries, the plant entries under
// Euler), k_rollout_plant.hip for WithRk4<model> (the plant entries under RK4).  The plant's integrator rides on the model
// type so that the kernels the policy and the params entries run keep their names and their code.
#pragma once
#include <cstdint>
#include "launchers.hpp"
#include "rollout_params_step.hpp"

namespace asif {

// M with the plant stepped by RK4 (plant_step.hpp): everything else of M as it is
template <class M>
struct WithRk4 : M {
	static constexpr int kPlant = kPlantRk4;
};
template <class M, class = void>
struct plant_of : std::integral_constant<int, kPlantEuler> {};
template <class M>
struct plant_of<M, std::enable_if_t<(M::kPlant >= 0)>> : std::integral_constant<int, M::kPlant> {};

// The value must be in its registers here: the wait for a load issued earlier is placed at this point.  The memory
// counter of gfx9 counts loads and stores in issue order, so a wait for a prefetched value that comes AFTER a step's
// stores also waits for those stores to be acknowledged -- several hundred cycles per step.  Placed in front of the
// stores, the wait covers only operations issued a whole solve earlier.
__device__ __forceinline__ void arrived(double &r) { asm volatile("" : "+v"(r)); }

// the handle's fields, then the instance's own where given; gainOk: param_gain_usable of a gain that was handed in
template <class M>
__device__ __forceinline__ RolloutVjpOpts<M::NU> lane_opts(const RolloutVjpOpts<M::NU> &e, const double *alpha,
                                                          const double *lb, const double *ub, int64_t ld, int64_t i,
                                                          bool &gainOk)
{
	RolloutVjpOpts<M::NU> el = e;
	if (alpha) el.relaxLb = alpha[i]; // wave-uniform, as the two below
#pragma unroll
	for (int j = 0; j < M::NU; j++) {
		if (lb) el.lb[j] = lb[j * ld + i];
		if (ub) el.ub[j] = ub[j * ld + i];
	}
	gainOk = alpha ? param_gain_usable(el.relaxLb) : true;
	return el;
}

// HASV: v is given.  Without it the loop holds no load, as explicit_rollout_kernel's.
// PARAMS: pa.alpha, pa.lb, pa.ub are looked at.  Without it el is e and gainOk is true.
// The plant's integrator (plant_step.hpp) is M's: plant_of<M>, Euler for a model as models.hpp defines it.
template <class M, bool HASV, bool PARAMS>
__global__ __launch_bounds__(256) void rollout_policy_kernel(RolloutVjpOpts<M::NU> e, ParamRolloutArgs pa)
{
	static_assert(M::kIgnoresOptions, "the model's functors must not read DevOptions: only the class's fields are passed");
	static_assert(M::NU == 1, "one input: the pinned relaxation variable leaves a one-variable problem");
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS, NV = NU + 1, NC = NP, PLANT = plant_of<M>::value;
	const PolicyRolloutArgs &a = pa.p;
	const DevOptions o = {};
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the wave votes of the solve; it never stores
	const int64_t ld = a.ld;
	const bool hasK = a.K != nullptr; // wave-uniform
	constexpr bool hasV = HASV;
	bool gainOk = true;
	RolloutVjpOpts<NU> el = e;
	if constexpr (PARAMS) el = lane_opts<M>(e, pa.alpha, pa.lb, pa.ub, ld, i, gainOk);
	double x[NX], uAct[NU], kk[NU], K[NU * NX], v[NU], vn[NU], relax;
#pragma unroll
	for (int k = 0; k < NX; k++) x[k] = a.x[k * ld + i];
#pragma unroll
	for (int j = 0; j < NU; j++) {
		kk[j] = a.k[j * ld + i];
		uAct[j] = a.uact[j * ld + i];
		v[j] = hasV ? a.v[j * ld + i] : 0.0; // T >= 1: the launcher does not launch otherwise
		vn[j] = 0.0;
	}
#pragma unroll
	for (int c = 0; c < NU * NX; c++) K[c] = hasK ? a.K[c * ld + i] : 0.0;
	relax = a.relax[i];
	int nfail = 0;
	if constexpr (HASV) { // the launch's own loads end here: a wait left at the loop's head would cover each step's stores
#pragma unroll
		for (int k = 0; k < NX; k++) arrived(x[k]);
#pragma unroll
		for (int j = 0; j < NU; j++) {
			arrived(kk[j]), arrived(uAct[j]), arrived(v[j]);
			if constexpr (PARAMS) arrived(el.lb[j]), arrived(el.ub[j]);
		}
#pragma unroll
		for (int c = 0; c < NU * NX; c++) arrived(K[c]);
		arrived(relax);
		if constexpr (PARAMS) arrived(el.relaxLb);
	}
#pragma unroll 1
	for (int t = 0; t < a.T; t++) { // wave-uniform trip count
		if (hasV && t + 1 < a.T) {
#pragma unroll
			for (int j = 0; j < NU; j++) vn[j] = a.v[((int64_t)(t + 1) * NU + j) * ld + i]; // in flight behind this step's solve
		}
		double uDes[NU];
		policy_udes<NX, NU>(kk, K, hasK, x, v, hasV, uDes);
		double h[NP], Dh[NP * NX], f[NX], gm[NX * NU];
		model_step_functors<M>(o, x, h, Dh, f, gm);
		QpLaneData<NV, NC> qp;
		explicit_step_qp<NX, NU, NP>(h, Dh, f, gm, uDes, el, qp);
		double sol[NV];
		int iters;
		const int verdict = GiSmall<NV, NC, 1>::template solve_with_pinned<NU>(qp, 0, 8 * NV + 4, sol, iters);
		if constexpr (HASV) {
#pragma unroll
			for (int j = 0; j < NU; j++) arrived(vn[j]); // in front of this step's stores
		}
		if (live && a.xlog) {
#pragma unroll
			for (int k = 0; k < NX; k++) a.xlog[((int64_t)t * NX + k) * ld + i] = x[k];
		}
		const bool ok = (verdict == kGiOptimal) & gainOk;
		// selects: written as `if (ok)`, whether the compiler if-converts the step's tail is left to its cost threshold
#pragma unroll
		for (int j = 0; j < NU; j++) uAct[j] = ok ? fmin(fmax(sol[j], el.lb[j]), el.ub[j]) : uAct[j];
		relax = ok ? sol[NU] : relax;
		nfail += ok ? 0 : 1;
		if (live && a.ulog) {
#pragma unroll
			for (int j = 0; j < NU; j++) a.ulog[((int64_t)t * NU + j) * ld + i] = uAct[j];
		}
		if (live && a.rclog) a.rclog[(int64_t)t * ld + i] = ok ? ASIF_HIP_RC_OK : ASIF_HIP_RC_QP_FAILED;
		if constexpr (PLANT == kPlantEuler) {
#pragma clang fp contract(off)
#pragma unroll
			for (int k = 0; k < NX; k++) {
				double fcl = 0.0;
				fcl += f[k];
#pragma unroll
				for (int j = 0; j < NU; j++) fcl += uAct[j] * gm[k + j * NX];
				x[k] += a.dt * fcl;
			}
		} else {
			plant_step<M, PLANT>(o, a.dt, f, gm, uAct, x);
		}
#pragma unroll
		for (int j = 0; j < NU; j++) v[j] = vn[j];
	}
	if (!live) return;
#pragma unroll
	for (int k = 0; k < NX; k++) a.x[k * ld + i] = x[k];
#pragma unroll
	for (int j = 0; j < NU; j++) a.uact[j * ld + i] = uAct[j];
	a.relax[i] = relax;
	a.nfail[i] = nfail;
}

template <class M>
struct PolicyStepLogs {
	double x[M::NX], u[M::NU], gx[M::NX], gu[M::NU], v[M::NU];
	int rc;
};

template <class M>
__device__ __forceinline__ void load_policy_step(const PolicyRolloutVjpArgs &a, int t, int64_t i, PolicyStepLogs<M> &L)
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
		L.v[j] = a.v ? a.v[at] : 0.0;
	}
	L.rc = a.rclog[(int64_t)t * a.ld + i];
}

// PARAMS: as the forward kernel's.  WANTP: one of pa.galpha, pa.glb, pa.gub is given (PARAMS only).
template <class M, bool PARAMS, bool WANTP>
__global__ __launch_bounds__(256) void rollout_policy_vjp_kernel(RolloutVjpOpts<M::NU> e, ParamRolloutVjpArgs pa)
{
	static_assert(M::kIgnoresOptions, "the model's functors must not read DevOptions: only the class's fields are passed");
	static_assert(PARAMS || !WANTP, "a parameter gradient belongs to a parameter");
	constexpr int NX = M::NX, NU = M::NU, PLANT = plant_of<M>::value;
	const PolicyRolloutVjpArgs &a = pa.p;
	const DevOptions o = {};
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the wave votes of the solve; it never stores
	const bool hasK = a.K != nullptr, hasV = a.v != nullptr; // wave-uniform
	bool gainOk; // the forward pass's business: a step it failed is rc -1 in the log
	RolloutVjpOpts<NU> el = e;
	if constexpr (PARAMS) el = lane_opts<M>(e, pa.alpha, pa.lb, pa.ub, a.ld, i, gainOk);

	double kk[NU], K[NU * NX];
	ParamAdjoint<M> q;
	PolicyAdjoint<M> &p = q.p;
#pragma unroll
	for (int k = 0; k < NX; k++) p.s.lam[k] = a.gxT[k * a.ld + i];
#pragma unroll
	for (int j = 0; j < NU; j++) {
		kk[j] = a.k[j * a.ld + i];
		p.s.mu[j] = a.guactT ? a.guactT[j * a.ld + i] : 0.0;
		p.s.gudes[j] = 0.0;
		p.gk[j] = 0.0;
		q.glb[j] = 0.0;
		q.gub[j] = 0.0;
	}
#pragma unroll
	for (int c = 0; c < NU * NX; c++) {
		K[c] = hasK ? a.K[c * a.ld + i] : 0.0;
		p.gK[c] = 0.0;
	}
	p.s.nskip = 0;
	q.galpha = 0.0;

	PolicyStepLogs<M> cur = {}, nxt = {};
	if (a.T > 0) load_policy_step<M>(a, a.T - 1, i, cur);
#pragma unroll 1
	for (int t = a.T - 1; t >= 0; t--) { // wave-uniform trip count
		if (t > 0) load_policy_step<M>(a, t - 1, i, nxt); // in flight behind this step's solve
		rollout_params_vjp_step<M, PLANT>(o, el, a.dt, cur.x, cur.u, kk, K, hasK, cur.v, hasV, cur.rc, cur.gx, cur.gu, WANTP, q);
		if (live && a.gv) {
#pragma unroll
			for (int j = 0; j < NU; j++) a.gv[((int64_t)t * NU + j) * a.ld + i] = p.s.gudes[j];
		}
		cur = nxt;
	}
	if (!live) return;
#pragma unroll
	for (int k = 0; k < NX; k++) a.gx0[k * a.ld + i] = p.s.lam[k];
#pragma unroll
	for (int j = 0; j < NU; j++) {
		a.gk[j * a.ld + i] = p.gk[j];
		a.guact0[j * a.ld + i] = p.s.mu[j];
		if constexpr (PARAMS) {
			if (pa.glb) pa.glb[j * a.ld + i] = q.glb[j];
			if (pa.gub) pa.gub[j * a.ld + i] = q.gub[j];
		}
	}
	if (a.gK) {
#pragma unroll
		for (int c = 0; c < NU * NX; c++) a.gK[c * a.ld + i] = p.gK[c];
	}
	if constexpr (PARAMS) {
		if (pa.galpha) pa.galpha[i] = q.galpha;
	}
	a.nskip[i] = p.s.nskip;
}

// The launches, written once for both translation units: one instance per lane, 256-thread workgroups; HASV from a.p.v.
// Without an instance or a step the forward pass has nothing to do.
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

// T == 0 runs the kernel too (the identity).  WANTP where one of the three parameter gradients is asked for: without it
// the step hands nothing out and the loop is the policy entry's
template <class M, bool PARAMS>
static int launch_backward(const DevOptions &o, const ParamRolloutVjpArgs &a, hipStream_t stream)
{
	if (a.p.B <= 0) return 0;
	const dim3 grid(grid_for(a.p.B, 1, 256)), block(256);
	const RolloutVjpOpts<M::NU> e = rollout_class_opts<M>(o);
	if constexpr (PARAMS) {
		if (a.galpha || a.glb || a.gub) hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, true, true>), grid, block, 0, stream, e, a);
		else hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, true, false>), grid, block, 0, stream, e, a);
	} else {
		hipLaunchKernelGGL((rollout_policy_vjp_kernel<M, false, false>), grid, block, 0, stream, e, a);
	}
	return (int)hipGetLastError();
}

// launch_forward / launch_backward on WithRk4<model> with PARAMS: defined in k_rollout_plant.hip, where alone the RK4
// code is compiled, and called by the two launchers in k_rollout_policy.hip
int launch_rk4(int model, const DevOptions &o, const ParamRolloutArgs &a, hipStream_t stream);
int launch_rk4(int model, const DevOptions &o, const ParamRolloutVjpArgs &a, hipStream_t stream);

} // namespace asif
