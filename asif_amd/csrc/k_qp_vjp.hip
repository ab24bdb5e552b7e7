// k_qp_vjp.hip -- asif_hip_qp_solve_batch backwards for the shapes that run in registers (nv = 2, 3; up to 48 rows;
// diagonal cost): given dL/dx* of a scalar loss, the gradient with respect to Hd, c, A, b, lb and ub, for a batch, in
// one launch.  The adjoint itself is qp_vjp_small.hpp.
//
// The kernel repeats the solve -- GiSmall::solve_general<true>, the dual active-set method with its final working set
// handed out -- so nothing has to be kept between the two passes.  It calls solve_general directly, not solve():
// solve() eliminates a pinned variable only when EVERY problem of the wave pins it, so the path an instance takes,
// and with it the last bits of its working set, would depend on the instances it shares a wave with.
//
// Lane mapping as in the forward kernels (k_qp.hip, PaddedQpPolicy): G lanes per problem, the rows dealt round-robin
// (local row k of lane g is row g + k G), rows nc..NC-1 inert (0.x >= -1e20), variables, bounds and working set
// replicated.  Each lane stores the gradient of the rows it owns, lane 0 of the group everything else.
#include <cstdint>
#include "qp_vjp_small.hpp"
#include "launchers.hpp"

namespace asif {

template <int NV, int NC, int G>
__global__ __launch_bounds__(256) void qp_vjp_kernel(QpVjpArgs a)
{
	constexpr int RPL = (NC + G - 1) / G;
	const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int g = (int)(tid % G);
	int64_t i = tid / G;
	const bool live = i < a.B;
	if (!live) i = a.B - 1; // keep the lane in the group and wave operations of the solve; it never stores
	const int nc = a.nc;
	const int64_t ld = a.ld;

	QpLaneData<NV, RPL> qp;
	double gsol[NV];
#pragma unroll
	for (int j = 0; j < NV; j++) {
		qp.Hd[j] = a.Hd[j * ld + i];
		qp.c[j] = a.c[j * ld + i];
		qp.lb[j] = a.lb[j * ld + i];
		qp.ub[j] = a.ub[j * ld + i];
		gsol[j] = a.gsol[j * ld + i];
	}
#pragma unroll
	for (int k = 0; k < RPL; k++) {
		const int r = g + k * G;
		const bool valid = r < nc;
		const int rr = valid ? r : 0;
#pragma unroll
		for (int j = 0; j < NV; j++) {
			const double v = a.A[(int64_t)(rr + j * nc) * ld + i];
			qp.A[k][j] = valid ? v : 0.0;
		}
		const double bv = a.b[(int64_t)rr * ld + i];
		qp.b[k] = valid ? bv : -1e20;
		qp.eq[k] = valid && ((a.be_mask >> rr) & 1ull);
	}

	double x[NV];
	GiWorkingSet<NV> ws;
	const int32_t rc = qp_vjp_solve<NV, RPL, G>(qp, g, x, ws);
	const bool ok = rc == 1;
	QpAdjoint<NV> adj;
	qp_adjoint_solve<NV>(qp.Hd, ws, gsol, adj);

	if (!live) return;
	// selects on every value: gsol of an instance that is not solved may be non-finite
	if (a.gA || a.gb) {
#pragma unroll
		for (int k = 0; k < RPL; k++) {
			const int r = g + k * G;
			if (r < nc) {
				double gb, gA[NV];
				qp_adjoint_row<NV>(ws, adj, ok, r, qp.A[k], x, gb, gA);
				if (a.gb) a.gb[(int64_t)r * ld + i] = gb;
				if (a.gA) {
#pragma unroll
					for (int j = 0; j < NV; j++) a.gA[(int64_t)(r + j * nc) * ld + i] = gA[j];
				}
			}
		}
	}
	if (g != 0) return;
	a.rc[i] = rc;
#pragma unroll
	for (int j = 0; j < NV; j++) {
		double glb, gub;
		qp_adjoint_bounds<NV>(ws, adj, j, glb, gub);
		if (a.gHd) a.gHd[j * ld + i] = ok ? -2.0 * x[j] * adj.z[j] : 0.0;
		if (a.gc) a.gc[j * ld + i] = ok ? 0.0 - adj.z[j] : 0.0;
		if (a.glb) a.glb[j * ld + i] = ok ? glb : 0.0;
		if (a.gub) a.gub[j * ld + i] = ok ? gub : 0.0;
		if (a.sol) a.sol[j * ld + i] = x[j];
	}
}

template <int NV, int NC, int G>
static int launch(const QpVjpArgs &a, hipStream_t stream)
{
	const int block = 256;
	hipLaunchKernelGGL((qp_vjp_kernel<NV, NC, G>), dim3(grid_for(a.B, G, block)), dim3(block), 0, stream, a);
	return (int)hipGetLastError();
}

// the instantiations follow the forward path's padded shapes: one lane per problem up to 8 rows, a lane group up to 48
int launch_qp_vjp(const QpVjpArgs &a, hipStream_t stream)
{
	if (a.B <= 0) return 0;
	if (a.nc < 1 || a.nc > 48 || a.B > 0x7fffffffLL) return ASIF_HIP_EUNSUPPORTED;
	if (a.nv == 2) return a.nc <= 8 ? launch<2, 8, 1>(a, stream) : launch<2, 48, 4>(a, stream);
	if (a.nv == 3) return a.nc <= 8 ? launch<3, 8, 1>(a, stream) : launch<3, 48, 4>(a, stream);
	return ASIF_HIP_EUNSUPPORTED;
}

} // namespace asif
