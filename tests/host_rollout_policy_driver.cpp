// host_rollout_policy_driver.cpp -- TEST HARNESS: the per-step adjoint of the fused explicit rollout under an affine
// policy (asif_amd/csrc/rollout_policy_step.hpp, one lane per instance) compiled with g++ and exposed through a C entry,
// so that tests/test_rollout_policy_ref_host.py can compare it with the numpy sweep of tests/rollout_policy_ref.py on the
// CPU.  It walks the batch and the steps the way rollout_policy_vjp_kernel (k_rollout_policy.hip) does.  models.hpp is
// device code; the double integrator's functors (examples/DoubleIntegrator.cpp:12-61 and their derivatives) are restated
// here in plain C++, as in host_rollout_vjp_driver.cpp.  Not part of any library the product ships.
#include <stdint.h>
#include "rollout_policy_step.hpp"

using namespace asif;

struct HostOpts {};

struct HostDoubleIntegrator {
	static constexpr int NX = 2, NU = 1, NPSS = 4;
	static void safetySet(const HostOpts &, const double (&x)[NX], double (&h)[NPSS], double (&Dh)[NPSS * NX])
	{
		const double xlo = -1.0, xhi = 1.0, vlo = -1.0, vhi = 1.0;
		const double brake = (x[1] * x[1]) / 2.0;
		const bool fwd = x[1] > 0;
		h[0] = fwd ? (xhi - x[0] - brake) : (-x[0] + xhi);
		h[1] = fwd ? (x[0] - xlo) : (x[0] - xlo - brake);
		h[2] = x[1] - vlo;
		h[3] = -x[1] + vhi;
		Dh[0] = -1.0; Dh[4] = fwd ? -x[1] : 0.0;
		Dh[1] = 1.0;  Dh[5] = fwd ? 0.0 : -x[1];
		Dh[2] = 0.0;  Dh[6] = 1.0;
		Dh[3] = 0.0;  Dh[7] = -1.0;
	}
	static void dynamics(const HostOpts &, const double (&x)[NX], double (&f)[NX], double (&g)[NX * NU])
	{
		f[0] = x[1];
		f[1] = 0.0;
		g[0] = 0.0;
		g[1] = 1.0;
	}
	static void safetyHess(const HostOpts &, const double (&x)[NX], double (&D2h)[NPSS * NX * NX])
	{
		const bool fwd = x[1] > 0;
		for (int k = 0; k < NPSS * NX * NX; k++) D2h[k] = 0.0;
		D2h[0 + NPSS * (1 + NX * 1)] = fwd ? -1.0 : 0.0;
		D2h[1 + NPSS * (1 + NX * 1)] = fwd ? 0.0 : -1.0;
	}
	static void dynamicsJac(const HostOpts &, const double (&)[NX], double (&Df)[NX * NX], double (&Dg)[NX * NX * NU])
	{
		Df[0] = 0.0; Df[2] = 1.0;
		Df[1] = 0.0; Df[3] = 0.0;
		for (int k = 0; k < NX * NX * NU; k++) Dg[k] = 0.0;
	}
};

// SoA buffers of leading dimension B, laid out as asif_hip_rollout_policy_vjp_batch takes them; K, v, guactT, gxlog, gulog,
// gK, gv may be null
extern "C" int rollout_policy_vjp_host_batch(int64_t B, int32_t T, double dt, int32_t npKeep, double lb, double ub,
                                             double relaxCost, double relaxLb, const double *xlog, const double *ulog,
                                             const int32_t *rclog, const double *K, const double *k, const double *v,
                                             const double *gxT, const double *guactT, const double *gxlog,
                                             const double *gulog, double *gx0, double *gK, double *gk, double *gv,
                                             double *guact0, int32_t *nskip)
{
	using M = HostDoubleIntegrator;
	constexpr int NX = M::NX, NU = M::NU;
	if ((gK && !K) || (gv && !v)) return -1;
	const HostOpts o;
	RolloutVjpOpts<NU> e;
	e.lb[0] = lb;
	e.ub[0] = ub;
	e.relaxCost = relaxCost;
	e.relaxLb = relaxLb;
	e.npKeep = npKeep < M::NPSS ? npKeep : M::NPSS;
	for (int64_t i = 0; i < B; i++) {
		PolicyAdjoint<M> p;
		double kk[NU], Kk[NU * NX];
		for (int m = 0; m < NX; m++) p.s.lam[m] = gxT[m * B + i];
		for (int j = 0; j < NU; j++) {
			kk[j] = k[j * B + i];
			p.s.mu[j] = guactT ? guactT[j * B + i] : 0.0;
			p.s.gudes[j] = 0.0;
			p.gk[j] = 0.0;
		}
		for (int c = 0; c < NU * NX; c++) {
			Kk[c] = K ? K[c * B + i] : 0.0;
			p.gK[c] = 0.0;
		}
		p.s.nskip = 0;
		for (int t = T - 1; t >= 0; t--) {
			double x[NX], u[NU], gx[NX], gu[NU], vt[NU];
			for (int m = 0; m < NX; m++) {
				const int64_t at = ((int64_t)t * NX + m) * B + i;
				x[m] = xlog[at];
				gx[m] = gxlog ? gxlog[at] : 0.0;
			}
			for (int j = 0; j < NU; j++) {
				const int64_t at = ((int64_t)t * NU + j) * B + i;
				u[j] = ulog[at];
				gu[j] = gulog ? gulog[at] : 0.0;
				vt[j] = v ? v[at] : 0.0;
			}
			rollout_policy_vjp_step<M>(o, e, dt, x, u, kk, Kk, K != nullptr, vt, v != nullptr, rclog[(int64_t)t * B + i], gx,
			                           gu, p);
			if (gv)
				for (int j = 0; j < NU; j++) gv[((int64_t)t * NU + j) * B + i] = p.s.gudes[j];
		}
		for (int m = 0; m < NX; m++) gx0[m * B + i] = p.s.lam[m];
		for (int j = 0; j < NU; j++) {
			gk[j * B + i] = p.gk[j];
			guact0[j * B + i] = p.s.mu[j];
		}
		if (gK)
			for (int c = 0; c < NU * NX; c++) gK[c * B + i] = p.gK[c];
		nskip[i] = p.s.nskip;
	}
	return 0;
}
