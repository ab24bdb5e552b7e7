// explicit_filter.hpp -- the body and the general kernel of the fused explicit CBF filter (k_explicit.hip) and the launcher
// of its general instantiations, for the translation units that instantiate them: k_explicit.hip (DoubleIntegrator,
// PlanarTwoInput and the light kernels) and k_explicit_cp.hip (CartPendulum).  One translation unit per group of models
// keeps each group's code object, and with it the placement of its kernels, independent of the models added next to it.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include "admm_small.hpp"
#include "launchers.hpp"

namespace asif {

// PRE: the instantiation for problems the dual active-set stage is known to decide on its own (one input, default
// solver mode or asif_hip_solver::presolve): no ADMM / finish code, hence none of their register footprint.
// SEL: the optional paths of src/asif.cpp (npSSmax < npSS row selection, caller-supplied Lie derivatives) are
// compiled in; the default instantiation (every row, the model's own Lie derivatives) does not carry them.
template <class M, int G, bool PRE, bool SEL = false, bool WHOLE = false>
__device__ __forceinline__ void explicit_filter_body(const DevOptions &o, const asif_hip_solver &S, const FilterArgs &a,
                                                     bool assemble_only)
{
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS, NV = NU + 1, NC = NP;
	constexpr int RPL = (NC + G - 1) / G;
	const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int g = (int)(tid % G);
	int64_t i = tid / G;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the group reductions; it never stores

	double x[NX], uDes[NU];
#pragma unroll
	for (int k = 0; k < NX; k++) x[k] = a.x[k * a.ld + i];
#pragma unroll
	for (int k = 0; k < NU; k++) uDes[k] = a.udes[k * a.ld + i];

	double h[NP], Dh[NP * NX], f[NX], gm[NX * NU];
	M::safetySet(o, x, h, Dh);
	M::dynamics(o, x, f, gm);
	double Lfh[NP], Lgh[NP * NU];
#pragma unroll
	for (int r = 0; r < NP; r++) {
		double s = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) s += Dh[r + k * NP] * f[k];
		Lfh[r] = s;
#pragma unroll
		for (int j = 0; j < NU; j++) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < NX; k++) t += Dh[r + k * NP] * gm[k + j * NX];
			Lgh[r + j * NP] = t;
		}
	}
	// npSSmax < npSS: only the rows of the smallest h are kept, in ascending order of h (src/asif.cpp:250-268);
	// pos[r] = position of safety function r in that order (ties: lower index first), kept iff pos[r] < nkeep
	const int nkeep = SEL ? o.npKeep : NP;
	int pos[NP];
#pragma unroll
	for (int r = 0; r < NP; r++) pos[r] = r;
	if (SEL && nkeep < NP) { // wave-uniform
#pragma unroll
		for (int r = 0; r < NP; r++) {
			int p = 0;
#pragma unroll
			for (int q = 0; q < NP; q++) p += (h[q] < h[r] || (h[q] == h[r] && q < r)) ? 1 : 0;
			pos[r] = p;
		}
	}
	if (SEL && a.lfh) { // caller-supplied Lie derivatives, indexed by row position (src/asif.cpp:287-292)
#pragma unroll
		for (int r = 0; r < NP; r++) {
			const int p = pos[r] < nkeep ? pos[r] : 0;
			Lfh[r] = a.lfh[(int64_t)p * a.ld + i];
#pragma unroll
			for (int j = 0; j < NU; j++) Lgh[r + j * NP] = a.lgh[(int64_t)(p + j * nkeep) * a.ld + i];
		}
	}
	if (assemble_only) {
		if (live && g == 0) {
#pragma unroll
			for (int r = 0; r < NP; r++) {
				if (pos[r] < nkeep) {
					const int p = pos[r];
#pragma unroll
					for (int j = 0; j < NU; j++) a.A[(int64_t)(p + j * nkeep) * a.ld + i] = Lgh[r + j * NP];
					a.A[(int64_t)(p + NU * nkeep) * a.ld + i] = h[r];
					a.b[(int64_t)p * a.ld + i] = -Lfh[r];
				}
			}
			a.code[i] = 1;
			if (a.diag) // which safety function sits in each row
				for (int r = 0; r < NP; r++)
					if (pos[r] < nkeep) a.diag[(int64_t)pos[r] * a.ld + i] = (double)r;
		}
		return;
	}

	QpLaneData<NV, RPL> qp;
#pragma unroll
	for (int j = 0; j < NU; j++) {
		qp.Hd[j] = 1.0;
		qp.c[j] = -2.0 * uDes[j];
		qp.lb[j] = o.lb[j];
		qp.ub[j] = o.ub[j];
	}
	qp.Hd[NU] = o.relaxCost;
	qp.c[NU] = -2.0 * o.relaxCost * o.relaxLb;
	qp.lb[NU] = o.relaxLb;
	qp.ub[NU] = o.relaxLb; // src/asif.cpp:91: the explicit class pins the relaxation variable
#pragma unroll
	for (int k = 0; k < RPL; k++) {
		// row r = g + k*G of the NC rows; out-of-range rows are inert (0.x >= -big)
#pragma unroll
		for (int j = 0; j < NV; j++) qp.A[k][j] = 0.0;
		qp.b[k] = -1e20;
		qp.eq[k] = false;
#pragma unroll
		for (int r = 0; r < NC; r++)
			if (r == g + k * G && pos[r] < nkeep) {
#pragma unroll
				for (int j = 0; j < NU; j++) qp.A[k][j] = Lgh[r + j * NP];
				qp.A[k][NU] = h[r];
				qp.b[k] = -Lfh[r];
			}
	}
	if constexpr (PRE) {
		static_assert(NU == 1 && G == 1, "one input: the pinned relaxation variable leaves a one-variable problem");
		// The explicit class pins its relaxation variable (lb = ub = relaxLb, src/asif.cpp:88-91): the dual active-set
		// stage eliminates it and what is left has one variable, which that stage always decides (gi_small.hpp:
		// solve_1d -- optimal or infeasible, never "undecided").  This instantiation therefore carries neither the ADMM
		// iterations nor the finish: 40 VGPRs instead of 256 + AGPRs, eight waves per SIMD instead of one.
		double sol[NV];
		int steps;
		const int verdict = GiSmall<NV, RPL, G>::template solve_with_pinned<NU>(qp, g, 8 * NV + 4, sol, steps);
		if constexpr (WHOLE) {
			// whole-line stores (see launch_explicit_di): a failed lane stores back what it finds in its slot
			const bool ok = verdict == kGiOptimal;
			double u = fmin(fmax(sol[0], o.lb[0]), o.ub[0]), rl = sol[NU];
			if (__any(live & !ok)) {
				if (live & !ok) {
					u = a.uact[i];
					rl = a.relax[i];
				}
			}
			if (live) {
				a.uact[i] = u;
				a.relax[i] = rl;
				a.rc[i] = ok ? ASIF_HIP_RC_OK : ASIF_HIP_RC_QP_FAILED;
			}
		} else if (live) {
			if (verdict == kGiOptimal) {
				a.uact[i] = fmin(fmax(sol[0], o.lb[0]), o.ub[0]);
				a.relax[i] = sol[NU];
				a.rc[i] = ASIF_HIP_RC_OK;
			} else {
				a.rc[i] = ASIF_HIP_RC_QP_FAILED; // uAct and relax stay untouched, src/asif.cpp:208-209
			}
		}
		if (live) {
			if (a.diag) {
				a.diag[0 * a.ld + i] = 0.0;
				a.diag[1 * a.ld + i] = 0.0;
				a.diag[(a.ndiag - 1) * a.ld + i] = 0.0;
			}
		}
		return;
	}

	AdmmSmall<NV, RPL, G> admm;
	double sol[NV];
	int status, iters;
	admm.solve(qp, S, sol, status, iters, false, S.polish != 1);

	if (live && g == 0) {
		if (status == kStatusSolved) {
#pragma unroll
			for (int j = 0; j < NU; j++) a.uact[j * a.ld + i] = fmin(fmax(sol[j], o.lb[j]), o.ub[j]);
			a.relax[i] = sol[NU];
			a.rc[i] = ASIF_HIP_RC_OK;
		} else {
			a.rc[i] = ASIF_HIP_RC_QP_FAILED; // uAct and relax stay untouched, src/asif.cpp:208-209
		}
		if (a.diag) {
			a.diag[0 * a.ld + i] = (double)admm.stat_rounds;
			a.diag[1 * a.ld + i] = (double)admm.stat_farkas;
			a.diag[(a.ndiag - 1) * a.ld + i] = (double)iters;
		}
	}
}

template <class M, int G, bool PRE, bool SEL = false>
__global__ __launch_bounds__((PRE ? 256 : 64), (G >= 2 ? 2 : 1)) void explicit_filter_kernel(DevOptions o, asif_hip_solver S, FilterArgs a,
                                                             bool assemble_only)
{
	explicit_filter_body<M, G, PRE, SEL>(o, S, a, assemble_only);
}

template <class M, int G>
static int launch_g(const DevOptions &o, const asif_hip_solver &S0, const FilterArgs &a, bool assemble_only,
                    hipStream_t stream)
{
	const int block = 64;
	// one Ruiz pass by default: the rows are well scaled and a second pass only costs finish rounds
	const asif_hip_solver S = resolve_scaling(S0, 1, 1);
	const bool sel = o.npKeep < M::NPSS || a.lfh != nullptr;
	if (sel)
		hipLaunchKernelGGL((explicit_filter_kernel<M, G, false, true>), dim3(grid_for(a.B, G, block)), dim3(block), 0,
		                   stream, o, S, a, assemble_only);
	else
		hipLaunchKernelGGL((explicit_filter_kernel<M, G, false, false>), dim3(grid_for(a.B, G, block)), dim3(block), 0,
		                   stream, o, S, a, assemble_only);
	return (int)hipGetLastError();
}

} // namespace asif
