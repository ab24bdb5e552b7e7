// k_explicit_vjp.hip -- the explicit CBF filter backwards: given dL/duAct, the gradient of a scalar loss with respect
// to what went into ASIF::filter (src/asif.cpp:176-210), for a batch, in one launch.
//
// Per instance the forward pass projects uDes onto {G u >= r, lb <= u <= ub} with G = Lgh, r = -Lfh - h relaxLb (the
// relaxation variable is pinned, src/asif.cpp:88-91).  With W the working set the dual active-set method ends with
// (bounds counted as rows +-e_j; |W| <= nu, linearly independent), lambda its multipliers and gbar = dL/duAct, the
// adjoint system  2 z + G_W' w = gbar,  G_W z = 0  gives
//     dL/duDes = 2 z,   dL/dr_k = w_k,   dL/dG_k = lambda_k z' - w_k u*'   (rows k in W; zero elsewhere),
//     dL/dLfh_k = -w_k,  dL/dLgh_k = dL/dG_k,  dL/dh_k = -relaxLb w_k,  dL/dx = Dh' dL/dh.
// |W| = nu: z = 0 and N' w = gbar is a square system (Cramer on the normals themselves);  |W| = 1 < nu:
// w = n.gbar / n.n,  z = (gbar - n w) / 2;  W empty: z = gbar / 2.  A constraint met with equality but outside W
// (multiplier zero) does not count: the one-sided derivative of the side the method ended on.
//
// The kernel repeats the forward pass up to the optimum -- same rows, same row selection, same dual active-set stage
// with the pinned variable eliminated (gi_small.hpp: solve_with_pinned_ws) -- so nothing has to be kept between the
// two passes; one instance per lane, SoA, every load and store a coalesced line, no ADMM / finish code.
#include <cstdint>
#include "gi_small.hpp"
#include "launchers.hpp"

namespace asif {

struct ExplicitVjpOpts { // the fields of DevOptions the explicit class reads (see explicit_light_kernel)
	double lb[ASIF_HIP_MAX_NU], ub[ASIF_HIP_MAX_NU], relaxCost, relaxLb;
	int npKeep;
};

// LIE: caller-supplied Lie derivatives (src/asif.cpp:287-292) and their gradients; otherwise the model's own, and
// dL/duDes is the only output
template <class M, bool LIE>
__global__ __launch_bounds__(256) void explicit_vjp_kernel(ExplicitVjpOpts e, VjpArgs a)
{
	static_assert(M::kIgnoresOptions, "the model's functors must not read DevOptions: only the class's fields are passed");
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS, NV = NU + 1, NC = NP;
	static_assert(NU == 1 || NU == 2, "closed-form adjoint: 1 x 1 or 2 x 2");
	const DevOptions o = {};
	int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the wave votes of the solve; it never stores

	double x[NX], uDes[NU], gbar[NU];
#pragma unroll
	for (int k = 0; k < NX; k++) x[k] = a.x[k * a.ld + i];
#pragma unroll
	for (int k = 0; k < NU; k++) {
		uDes[k] = a.udes[k * a.ld + i];
		gbar[k] = a.guact[k * a.ld + i];
	}

	// ---- 1. the rows, as explicit_filter_body assembles them
	double h[NP], Dh[NP * NX], Lfh[NP], Lgh[NP * NU];
	M::safetySet(o, x, h, Dh);
	if constexpr (!LIE) {
		double f[NX], gm[NX * NU];
		M::dynamics(o, x, f, gm);
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
	}
	// npSSmax < npSS: the rows of the nkeep smallest h, in ascending order of h (ties: lower index first)
	const int nkeep = e.npKeep;
	int pos[NP];
#pragma unroll
	for (int r = 0; r < NP; r++) pos[r] = r;
	if (nkeep < NP) { // wave-uniform
#pragma unroll
		for (int r = 0; r < NP; r++) {
			int p = 0;
#pragma unroll
			for (int q = 0; q < NP; q++) p += (h[q] < h[r] || (h[q] == h[r] && q < r)) ? 1 : 0;
			pos[r] = p;
		}
	}
	if constexpr (LIE) { // indexed by row position
#pragma unroll
		for (int r = 0; r < NP; r++) {
			const int p = pos[r] < nkeep ? pos[r] : 0;
			Lfh[r] = a.lfh[(int64_t)p * a.ld + i];
#pragma unroll
			for (int j = 0; j < NU; j++) Lgh[r + j * NP] = a.lgh[(int64_t)(p + j * nkeep) * a.ld + i];
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
	for (int r = 0; r < NC; r++) { // dropped rows are inert (0.x >= -big)
		const bool kept = pos[r] < nkeep;
#pragma unroll
		for (int j = 0; j < NU; j++) qp.A[r][j] = kept ? Lgh[r + j * NP] : 0.0;
		qp.A[r][NU] = kept ? h[r] : 0.0;
		qp.b[r] = kept ? -Lfh[r] : -1e20;
		qp.eq[r] = false;
	}

	// ---- 2. / 3. the forward solve, and the working set it ends with
	double sol[NV];
	int steps;
	GiWorkingSet<NU> ws;
	const int verdict = GiSmall<NV, NC, 1>::template solve_with_pinned_ws<NU>(qp, 0, 8 * NV + 4, sol, steps, ws);
	const bool ok = verdict == kGiOptimal;
	const int32_t rc = ok ? ASIF_HIP_RC_OK : (verdict == kGiUndecided ? 0 : ASIF_HIP_RC_QP_FAILED);

	// ---- 4. the adjoint.  w[s] belongs to slot s; the normal of an empty slot is zero
	double u[NU], w[NU], z[NU];
#pragma unroll
	for (int j = 0; j < NU; j++) u[j] = fmin(fmax(sol[j], e.lb[j]), e.ub[j]); // inputSaturate, src/asif.cpp:343-352
	if constexpr (NU == 1) {
		const bool in = ws.id[0] >= 0;
		w[0] = in ? gbar[0] / ws.nrm[0][0] : 0.0;
		z[0] = in ? 0.0 : 0.5 * gbar[0];
	} else {
		const double(&n0)[2] = ws.nrm[0], (&n1)[2] = ws.nrm[1];
		const bool v0 = ws.id[0] >= 0, v1 = ws.id[1] >= 0, both = v0 & v1, one = v0 != v1;
		const double det = n0[0] * n1[1] - n1[0] * n0[1];
		const double m[2] = {n0[0] + n1[0], n0[1] + n1[1]}; // the one normal when `one`
		const double mm = m[0] * m[0] + m[1] * m[1];
		const double w1d = (m[0] * gbar[0] + m[1] * gbar[1]) / (one ? mm : 1.0);
		const double idet = 1.0 / (both ? det : 1.0);
		w[0] = both ? (gbar[0] * n1[1] - n1[0] * gbar[1]) * idet : ((one & v0) ? w1d : 0.0);
		w[1] = both ? (n0[0] * gbar[1] - gbar[0] * n0[1]) * idet : ((one & v1) ? w1d : 0.0);
#pragma unroll
		for (int j = 0; j < 2; j++) z[j] = both ? 0.0 : 0.5 * (gbar[j] - w[0] * n0[j] - w[1] * n1[j]);
	}
	if (!live) return;
	a.rc[i] = rc;
#pragma unroll
	for (int j = 0; j < NU; j++) a.gudes[j * a.ld + i] = ok ? 2.0 * z[j] : 0.0;
	if constexpr (LIE) {
		double wr[NP], lr[NP]; // per safety function: w and lambda of its row, zero outside W
#pragma unroll
		for (int r = 0; r < NP; r++) {
			wr[r] = 0.0;
			lr[r] = 0.0;
#pragma unroll
			for (int s = 0; s < NU; s++) {
				const bool mine = ok & (ws.id[s] == r);
				wr[r] = mine ? w[s] : wr[r];
				lr[r] = mine ? ws.lam[s] : lr[r];
			}
		}
		if (a.glfh) {
#pragma unroll
			for (int r = 0; r < NP; r++)
				if (pos[r] < nkeep) a.glfh[(int64_t)pos[r] * a.ld + i] = 0.0 - wr[r];
		}
		if (a.glgh) {
#pragma unroll
			for (int r = 0; r < NP; r++)
				if (pos[r] < nkeep) {
#pragma unroll
					for (int j = 0; j < NU; j++)
						a.glgh[(int64_t)(pos[r] + j * nkeep) * a.ld + i] = ok ? lr[r] * z[j] - wr[r] * u[j] : 0.0;
				}
		}
		if (a.gx) { // x reaches the rows through h alone here: dL/dh_k = -relaxLb w_k
#pragma unroll
			for (int k = 0; k < NX; k++) {
				double s = 0.0;
#pragma unroll
				for (int r = 0; r < NP; r++) s += Dh[r + k * NP] * wr[r];
				a.gx[k * a.ld + i] = ok ? 0.0 - e.relaxLb * s : 0.0; // selects: a failed instance may hold non-finite data
			}
		}
	}
}

template <class M>
static int launch_vjp(const DevOptions &o, const VjpArgs &a, hipStream_t stream)
{
	if (a.B <= 0) return 0;
	const int block = 256;
	ExplicitVjpOpts e;
	for (int j = 0; j < ASIF_HIP_MAX_NU; j++) {
		e.lb[j] = o.lb[j];
		e.ub[j] = o.ub[j];
	}
	e.relaxCost = o.relaxCost;
	e.relaxLb = o.relaxLb;
	e.npKeep = o.npKeep < M::NPSS ? o.npKeep : M::NPSS;
	if (a.lfh)
		hipLaunchKernelGGL((explicit_vjp_kernel<M, true>), dim3(grid_for(a.B, 1, block)), dim3(block), 0, stream, e, a);
	else
		hipLaunchKernelGGL((explicit_vjp_kernel<M, false>), dim3(grid_for(a.B, 1, block)), dim3(block), 0, stream, e, a);
	return (int)hipGetLastError();
}

int launch_explicit_vjp_di(const DevOptions &o, const VjpArgs &a, hipStream_t stream)
{
	return launch_vjp<DoubleIntegrator>(o, a, stream);
}
int launch_explicit_vjp_p2(const DevOptions &o, const VjpArgs &a, hipStream_t stream)
{
	return launch_vjp<PlanarTwoInput>(o, a, stream);
}
int launch_explicit_vjp_cp(const DevOptions &o, const VjpArgs &a, hipStream_t stream)
{
	return launch_vjp<CartPendulum>(o, a, stream);
}

} // namespace asif
