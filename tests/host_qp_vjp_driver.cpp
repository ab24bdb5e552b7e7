// host_qp_vjp_driver.cpp -- TEST HARNESS: the adjoint of the in-register QP solve (asif_amd/csrc/qp_vjp_small.hpp on top
// of GiSmall::solve_general<true>, one lane per QP) compiled with g++ and exposed through a C entry, so that
// tests/test_qp_vjp_host.py can compare it with the numpy adjoint of tests/qp_vjp_ref.py on the CPU.  It walks the
// batch the way qp_vjp_kernel (k_qp_vjp.hip) walks its lanes.  Not part of any library the product ships.
#include <stdint.h>
#include "qp_vjp_small.hpp"

using namespace asif;

template <int NV, int NC>
static void run(int64_t B, int nc, const double *Hd, const double *c, const double *A, const double *b, const double *lb,
                const double *ub, const uint8_t *be, const double *gsol, double *gHd, double *gc, double *gA, double *gb,
                double *glb, double *gub, double *sol, int32_t *rc)
{
	for (int64_t i = 0; i < B; i++) {
		QpLaneData<NV, NC> qp;
		double g[NV];
		for (int j = 0; j < NV; j++) {
			qp.Hd[j] = Hd[i * NV + j];
			qp.c[j] = c[i * NV + j];
			qp.lb[j] = lb[i * NV + j];
			qp.ub[j] = ub[i * NV + j];
			g[j] = gsol[i * NV + j];
		}
		for (int r = 0; r < NC; r++) {
			const bool valid = r < nc;
			for (int j = 0; j < NV; j++) qp.A[r][j] = valid ? A[i * nc * NV + r + j * nc] : 0.0; // col-major nc x nv
			qp.b[r] = valid ? b[i * nc + r] : -1e20;
			qp.eq[r] = valid && be && be[r];
		}
		double x[NV];
		GiWorkingSet<NV> ws;
		const int v = qp_vjp_solve<NV, NC, 1>(qp, 0, x, ws);
		const bool ok = v == 1;
		QpAdjoint<NV> adj;
		qp_adjoint_solve<NV>(qp.Hd, ws, g, adj);
		rc[i] = v;
		for (int r = 0; r < nc; r++) {
			double gbr, gAr[NV];
			qp_adjoint_row<NV>(ws, adj, ok, r, qp.A[r], x, gbr, gAr);
			gb[i * nc + r] = gbr;
			for (int j = 0; j < NV; j++) gA[i * nc * NV + r + j * nc] = gAr[j];
		}
		for (int j = 0; j < NV; j++) {
			double l, u;
			qp_adjoint_bounds<NV>(ws, adj, j, l, u);
			gHd[i * NV + j] = ok ? -2.0 * x[j] * adj.z[j] : 0.0;
			gc[i * NV + j] = ok ? 0.0 - adj.z[j] : 0.0;
			glb[i * NV + j] = ok ? l : 0.0;
			gub[i * NV + j] = ok ? u : 0.0;
			sol[i * NV + j] = x[j];
		}
	}
}

// AoS per instance like the oracle's or_qp_solve_batch: Hd[nv], c[nv], A[nc*nv] col-major, b[nc], lb[nv], ub[nv],
// gsol[nv]; gradients in the same shapes.  rc as asif_hip_qp_vjp_batch writes it.  Returns 0, or -1 for a shape
// without an instantiation.
extern "C" int qp_vjp_host_batch(int nv, int nc, int64_t B, const double *Hd, const double *c, const double *A,
                                 const double *b, const double *lb, const double *ub, const uint8_t *be,
                                 const double *gsol, double *gHd, double *gc, double *gA, double *gb, double *glb,
                                 double *gub, double *sol, int32_t *rc)
{
#define SHAPE(NV_, NC_) \
	if (nv == NV_ && nc >= 1 && nc <= NC_) { \
		run<NV_, NC_>(B, nc, Hd, c, A, b, lb, ub, be, gsol, gHd, gc, gA, gb, glb, gub, sol, rc); \
		return 0; \
	}
	SHAPE(2, 8)
	SHAPE(2, 48)
	SHAPE(3, 8)
	SHAPE(3, 48)
#undef SHAPE
	return -1;
}
