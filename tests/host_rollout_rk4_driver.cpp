// host_rollout_rk4_driver.cpp -- TEST HARNESS: the plant's step and its adjoint (asif_amd/csrc/plant_step.hpp) and the
// per-step adjoint of the fused rollout around them (rollout_params_step.hpp with the integrator as its compile-time
// argument), compiled with g++ and exposed through two C entries, so that tests/test_rollout_rk4_ref_host.py can compare
// them with the numpy step and sweep of tests/rollout_rk4_ref.py on the CPU.  The sweep walks the batch and the steps the
// way rollout_policy_vjp_kernel with PARAMS (rollout_policy_kernels.hpp) does.  models.hpp is device code; the functors of
// both models are restated here in plain C++, as in host_rollout_params_driver.cpp and host_cart_pendulum_driver.cpp,
// with the joint forms a stage of the plant's step calls.  Not part of any library the product ships.
// model: 0 the double integrator, 10 the cart-driven pendulum; integrator (of the sweep): 0 Euler, 1 RK4
// (ASIF_HIP_PLANT_*).  plant_step.hpp holds the RK4 step alone: the step entry is RK4.
// With -DRK4_DRIVER_MAIN the file is a stand-alone program (for a sanitizer build of the host code): it runs a small
// batch of both models under both integrators through every combination of absent inputs and outputs and prints a
// checksum.
#include <cmath>
#include <stdint.h>
#include "rollout_params_step.hpp"

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

struct HostCartPendulum {
	static constexpr int NX = 2, NU = 1, NPSS = 4;
	static constexpr bool kJointFunctors = true;
	static void safetySetAt(double s, double c, const double (&x)[NX], double (&h)[NPSS], double (&Dh)[NPSS * NX])
	{
		const double brake = (x[1] * x[1]) / 2.0;
		const bool fwd = x[1] > 0;
		h[0] = fwd ? (1.0 - x[0] - brake) : (-x[0] + 1.0);
		h[1] = fwd ? (x[0] + 1.0) : (x[0] + 1.0 - brake);
		h[2] = 1.5 - ((x[0] * x[0] + x[0] * x[1]) + x[1] * x[1]);
		h[3] = c - brake;
		Dh[0] = -1.0;                 Dh[4] = fwd ? -x[1] : 0.0;
		Dh[1] = 1.0;                  Dh[5] = fwd ? 0.0 : -x[1];
		Dh[2] = -(2.0 * x[0] + x[1]); Dh[6] = -(x[0] + 2.0 * x[1]);
		Dh[3] = -s;                   Dh[7] = -x[1];
	}
	static void stepFunctors(const HostOpts &, const double (&x)[NX], double (&h)[NPSS], double (&Dh)[NPSS * NX],
	                         double (&f)[NX], double (&g)[NX * NU])
	{
		const double s = std::sin(x[0]), c = std::cos(x[0]);
		safetySetAt(s, c, x, h, Dh);
		f[0] = x[1];
		f[1] = s;
		g[0] = 0.0;
		g[1] = -c;
	}
	static void adjointFunctors(const HostOpts &o, const double (&x)[NX], double (&h)[NPSS], double (&Dh)[NPSS * NX],
	                            double (&f)[NX], double (&g)[NX * NU], double (&D2h)[NPSS * NX * NX], double (&Df)[NX * NX],
	                            double (&Dg)[NX * NX * NU])
	{
		stepFunctors(o, x, h, Dh, f, g);
		const double s = f[1], c = -g[1];
		const bool fwd = x[1] > 0;
		for (int k = 0; k < NPSS * NX * NX; k++) D2h[k] = 0.0;
		D2h[0 + NPSS * (1 + NX * 1)] = fwd ? -1.0 : 0.0;
		D2h[1 + NPSS * (1 + NX * 1)] = fwd ? 0.0 : -1.0;
		D2h[2 + NPSS * (0 + NX * 0)] = -2.0;
		D2h[2 + NPSS * (1 + NX * 0)] = -1.0;
		D2h[2 + NPSS * (0 + NX * 1)] = -1.0;
		D2h[2 + NPSS * (1 + NX * 1)] = -2.0;
		D2h[3 + NPSS * (0 + NX * 0)] = -c;
		D2h[3 + NPSS * (1 + NX * 1)] = -1.0;
		Df[0] = 0.0; Df[2] = 1.0;
		Df[1] = c;   Df[3] = 0.0;
		for (int k = 0; k < NX * NX * NU; k++) Dg[k] = 0.0;
		Dg[1] = s;
	}
	static void plantFunctors(const HostOpts &, const double (&x)[NX], double (&f)[NX], double (&g)[NX * NU])
	{
		const double s = std::sin(x[0]), c = std::cos(x[0]);
		f[0] = x[1];
		f[1] = s;
		g[0] = 0.0;
		g[1] = -c;
	}
	static void plantAdjointFunctors(const HostOpts &o, const double (&x)[NX], double (&f)[NX], double (&g)[NX * NU],
	                                 double (&Df)[NX * NX], double (&Dg)[NX * NX * NU])
	{
		plantFunctors(o, x, f, g);
		const double s = f[1], c = -g[1];
		Df[0] = 0.0; Df[2] = 1.0;
		Df[1] = c;   Df[3] = 0.0;
		for (int k = 0; k < NX * NX * NU; k++) Dg[k] = 0.0;
		Dg[1] = s;
	}
};

// x [nx][B] -> xn [nx][B] by one RK4 step under the held u [nu][B]: k1 from the model's f, g at x, as the forward kernel
// forms it
template <class M>
static void plant_step_batch(int64_t B, double dt, const double *x, const double *u, double *xn)
{
	constexpr int NX = M::NX, NU = M::NU, NP = M::NPSS;
	const HostOpts o;
	for (int64_t i = 0; i < B; i++) {
		double xi[NX], ui[NU], h[NP], Dh[NP * NX], f[NX], gm[NX * NU];
		for (int m = 0; m < NX; m++) xi[m] = x[m * B + i];
		for (int j = 0; j < NU; j++) ui[j] = u[j * B + i];
		model_step_functors<M>(o, xi, h, Dh, f, gm);
		plant_step<M, kPlantRk4>(o, dt, f, gm, ui, xi);
		for (int m = 0; m < NX; m++) xn[m * B + i] = xi[m];
	}
}

template <class M, int PLANT>
static void sweep_batch(int64_t B, int32_t T, double dt, int32_t npKeep, double lb, double ub, double relaxCost,
                        double relaxLb, const double *xlog, const double *ulog, const int32_t *rclog, const double *K,
                        const double *k, const double *v, const double *alpha, const double *lbv, const double *ubv,
                        const double *gxT, const double *guactT, const double *gxlog, const double *gulog, double *gx0,
                        double *gK, double *gk, double *gv, double *galpha, double *glb, double *gub, double *guact0,
                        int32_t *nskip)
{
	constexpr int NX = M::NX, NU = M::NU;
	const HostOpts o;
	const bool wantP = galpha || glb || gub;
	for (int64_t i = 0; i < B; i++) {
		RolloutVjpOpts<NU> e;
		e.lb[0] = lbv ? lbv[i] : lb;
		e.ub[0] = ubv ? ubv[i] : ub;
		e.relaxCost = relaxCost;
		e.relaxLb = alpha ? alpha[i] : relaxLb;
		e.npKeep = npKeep < M::NPSS ? npKeep : M::NPSS;
		ParamAdjoint<M> q;
		PolicyAdjoint<M> &p = q.p;
		double kk[NU], Kk[NU * NX];
		for (int m = 0; m < NX; m++) p.s.lam[m] = gxT[m * B + i];
		for (int j = 0; j < NU; j++) {
			kk[j] = k[j * B + i];
			p.s.mu[j] = guactT ? guactT[j * B + i] : 0.0;
			p.s.gudes[j] = 0.0;
			p.gk[j] = 0.0;
			q.glb[j] = 0.0;
			q.gub[j] = 0.0;
		}
		for (int c = 0; c < NU * NX; c++) {
			Kk[c] = K ? K[c * B + i] : 0.0;
			p.gK[c] = 0.0;
		}
		p.s.nskip = 0;
		q.galpha = 0.0;
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
			rollout_params_vjp_step<M, PLANT>(o, e, dt, x, u, kk, Kk, K != nullptr, vt, v != nullptr, rclog[(int64_t)t * B + i], gx,
			                           gu, wantP, q);
			if (gv)
				for (int j = 0; j < NU; j++) gv[((int64_t)t * NU + j) * B + i] = p.s.gudes[j];
		}
		for (int m = 0; m < NX; m++) gx0[m * B + i] = p.s.lam[m];
		for (int j = 0; j < NU; j++) {
			gk[j * B + i] = p.gk[j];
			guact0[j * B + i] = p.s.mu[j];
			if (glb) glb[j * B + i] = q.glb[j];
			if (gub) gub[j * B + i] = q.gub[j];
		}
		if (gK)
			for (int c = 0; c < NU * NX; c++) gK[c * B + i] = p.gK[c];
		if (galpha) galpha[i] = q.galpha;
		nskip[i] = p.s.nskip;
	}
}

template <class F>
static int dispatch(int32_t model, int32_t integrator, F &&f)
{
	if (integrator != kPlantEuler && integrator != kPlantRk4) return -1;
	const bool rk4 = integrator == kPlantRk4;
	if (model == 0) return rk4 ? f(HostDoubleIntegrator{}, std::integral_constant<int, kPlantRk4>{})
		                       : f(HostDoubleIntegrator{}, std::integral_constant<int, kPlantEuler>{});
	if (model == 10) return rk4 ? f(HostCartPendulum{}, std::integral_constant<int, kPlantRk4>{})
		                        : f(HostCartPendulum{}, std::integral_constant<int, kPlantEuler>{});
	return -1;
}

extern "C" int plant_step_host_batch(int32_t model, int64_t B, double dt, const double *x, const double *u, double *xn)
{
	return dispatch(model, kPlantRk4, [&](auto m, auto) {
		plant_step_batch<decltype(m)>(B, dt, x, u, xn);
		return 0;
	});
}

// SoA buffers of leading dimension B, laid out as asif_hip_rollout_plant_vjp_batch takes them; K, v, alpha, lbv, ubv,
// guactT, gxlog, gulog, gK, gv, galpha, glb, gub may be null.  lb, ub, relaxLb: the handle's values.
extern "C" int rollout_rk4_vjp_host_batch(int32_t model, int32_t integrator, int64_t B, int32_t T, double dt,
                                          int32_t npKeep, double lb, double ub, double relaxCost, double relaxLb,
                                          const double *xlog, const double *ulog, const int32_t *rclog, const double *K,
                                          const double *k, const double *v, const double *alpha, const double *lbv,
                                          const double *ubv, const double *gxT, const double *guactT,
                                          const double *gxlog, const double *gulog, double *gx0, double *gK, double *gk,
                                          double *gv, double *galpha, double *glb, double *gub, double *guact0,
                                          int32_t *nskip)
{
	if ((gK && !K) || (gv && !v) || (galpha && !alpha) || (glb && !lbv) || (gub && !ubv)) return -1;
	return dispatch(model, integrator, [&](auto m, auto p) {
		sweep_batch<decltype(m), decltype(p)::value>(B, T, dt, npKeep, lb, ub, relaxCost, relaxLb, xlog, ulog, rclog, K, k, v,
		                                             alpha, lbv, ubv, gxT, guactT, gxlog, gulog, gx0, gK, gk, gv, galpha, glb,
		                                             gub, guact0, nskip);
		return 0;
	});
}

#ifdef RK4_DRIVER_MAIN
#include <cstdio>
#include <vector>
// a closed loop of its own making: the logs need not be a filter's for the memory accesses to be the kernel's
int main()
{
	const int64_t B = 37;
	const int32_t T = 5;
	std::vector<double> xlog(T * 2 * B), ulog(T * B), K(2 * B), k(B), v(T * B), al(B), lo(B), hi(B), gxT(2 * B), guT(B),
		gxl(T * 2 * B), gul(T * B), gx0(2 * B), gK(2 * B), gk(B), gv(T * B), ga(B), gl(B), gu(B), gu0(B);
	std::vector<int32_t> rc(T * B), nskip(B);
	uint64_t s = 88172645463325252ull;
	auto rnd = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
	for (auto *a : {&xlog, &ulog, &K, &k, &v, &gxT, &guT, &gxl, &gul})
		for (double &d : *a) d = rnd();
	for (int64_t i = 0; i < B; i++) al[i] = 5.0 + 3.0 * rnd(), lo[i] = -1.0 + 0.5 * rnd(), hi[i] = 1.0 + 0.5 * rnd();
	for (size_t i = 0; i < rc.size(); i++) rc[i] = (i % 7) ? 1 : -1;
	std::vector<double> xn(2 * B);
	double sum = 0.0;
	for (int pass = 0; pass < 4; pass++) {
		const int32_t model = (pass & 1) ? 10 : 0, plant = pass >> 1;
		if (plant_step_host_batch(model, B, 1e-2, xlog.data(), ulog.data(), xn.data())) return 1;
		for (double d : xn) sum += d;
		for (int mask = 0; mask < 64; mask++) {
			const bool hK = mask & 1, hV = mask & 2, hP = mask & 4, gP = (mask & 8) && hP, gl_ = mask & 16, gg = mask & 32;
			const int r = rollout_rk4_vjp_host_batch(
				model, plant, B, T, 1e-2, (mask & 3) == 3 ? 2 : 4, -1.0, 1.0, 1e4, 6.0, xlog.data(), ulog.data(), rc.data(), hK ? K.data() : nullptr,
				k.data(), hV ? v.data() : nullptr, hP ? al.data() : nullptr, hP ? lo.data() : nullptr, hP ? hi.data() : nullptr,
				gxT.data(), gg ? guT.data() : nullptr, gl_ ? gxl.data() : nullptr, gl_ ? gul.data() : nullptr, gx0.data(),
				hK && gg ? gK.data() : nullptr, gk.data(), hV && gg ? gv.data() : nullptr, gP ? ga.data() : nullptr,
				gP ? gl.data() : nullptr, gP ? gu.data() : nullptr, gu0.data(), nskip.data());
			if (r) return 1;
			for (int64_t i = 0; i < B; i++) sum += gx0[i] + gk[i] + gu0[i] + (gP ? ga[i] + gl[i] + gu[i] : 0.0);
		}
	}
	std::printf("checksum %.17g\n", sum);
	return 0;
}
#endif
