// plant_step.hpp -- the plant's step between two filter calls of the fused rollouts under a policy, and its adjoint, per
// instance and in registers.  The ONE statement of the RK4 step and of its adjoint for the forward kernel, the backward
// kernel's stage recomputation and the host driver of the tests (tests/rollout_rk4_ref.py restates it in numpy).  The
// Euler step and its adjoint are NOT here: they stay, once each, where the kernels have always had them
// (rollout_policy_kernels.hpp: the loop's tail; rollout_vjp_step.hpp: section 1), selected by the same PLANT argument.
//
// The input u = u_t is held over the control period (zero-order hold); F(X, u) = f(X) + g(X) u.
//     kPlantEuler:  x+ = x + dt F(x, u)                                   (not in this file)
//     kPlantRk4:    k1 = F(x, u);  k2 = F(x + dt/2 k1, u);  k3 = F(x + dt/2 k2, u);  k4 = F(x + dt k3, u)
//                   x+ = x + dt/6 (k1 + 2 k2 + 2 k3 + k4)
// k1 uses the f and g the step's filter was assembled from (model_step_functors at x_t): they are not evaluated again.
// Stages 2 to 4 need f and g alone, no safety set: a model with joint functors supplies plantFunctors (f, g on one sine /
// cosine pair) and plantAdjointFunctors (f, g, Df, Dg on one pair), every other model is called through dynamics and
// dynamicsJac.  The filter is evaluated once per step, at x_t: THE BARRIER CONDITION IS ENFORCED AT THE SAMPLE INSTANTS
// ONLY, under either integrator; nothing is claimed about the state between two samples.
//
// Evaluation order, no contraction (every product and every sum rounded on its own):
//     F_k(X)  = (0 + f_k) + u_0 g_k0 (+ u_1 g_k1 ...)              -- explicit_rollout_kernel's fCl
//     X2 = x + (0.5 dt) k1;   X3 = x + (0.5 dt) k2;   X4 = x + dt k3      (0.5 dt is exact)
//     x+ = x + (dt / 6) (((k1 + 2 k2) + 2 k3) + k4)                      (2 k is exact; dt / 6 is one division)
// The Euler step is x + dt F(x), the order the kernels have always used.
//
// Adjoint.  Given lambda = dL/dx_{t+1}, the stage states X_1 = x_t, X_2, X_3, X_4 recomputed from the logged (x_t, u_t) in
// the order above (the forward pass's bits), J_i = Df(X_i) + sum_j u_j Dg_j(X_i):
//     kb4 = dt/6 lambda;              Xb4 = J4' kb4
//     kb3 = dt/3 lambda + dt   Xb4;   Xb3 = J3' kb3
//     kb2 = dt/3 lambda + dt/2 Xb3;   Xb2 = J2' kb2
//     kb1 = dt/6 lambda + dt/2 Xb2;   Xb1 = J1' kb1
//     mu     += gul + sum_i g(X_i)' kb_i
//     lambda' = lambda + Xb1 + Xb2 + Xb3 + Xb4 + gxl
// This is the exact derivative of the discrete step (discretise, then differentiate), not a discretisation of the
// continuous adjoint.  Under kPlantEuler the two lines are mu += gul + dt g' lambda, lambda' = lambda + dt J1' lambda + gxl.
// The stage values are dead when the adjoint returns: nothing of them is live across the solve that follows it.
//
// Compiles for the host like rollout_vjp_step.hpp, which includes it.  No loop indexes a register array by a run-time value.
#pragma once
#include <type_traits>
#include "qp_lane.hpp"

namespace asif {

constexpr int kPlantEuler = 0, kPlantRk4 = 1; // ASIF_HIP_PLANT_EULER, ASIF_HIP_PLANT_RK4

// A model whose functors share work at a state (the cart-driven pendulum: one sine / cosine pair) declares
// kJointFunctors and supplies joint forms -- the same values as the functors one by one, evaluated together: stepFunctors
// and adjointFunctors (rollout_vjp_step.hpp), plantFunctors and plantAdjointFunctors (below).  Every other model is called
// functor by functor.
template <class M, class = void>
struct joint_functors : std::false_type {};
template <class M>
struct joint_functors<M, std::enable_if_t<M::kJointFunctors>> : std::true_type {};

template <class M, class O>
ASIF_HD void model_plant_functors(const O &o, const double (&x)[M::NX], double (&f)[M::NX], double (&gm)[M::NX * M::NU])
{
	if constexpr (joint_functors<M>::value) M::plantFunctors(o, x, f, gm);
	else M::dynamics(o, x, f, gm);
}

template <class M, class O>
ASIF_HD void model_plant_adjoint_functors(const O &o, const double (&x)[M::NX], double (&f)[M::NX],
                                          double (&gm)[M::NX * M::NU], double (&Df)[M::NX * M::NX],
                                          double (&Dg)[M::NX * M::NX * M::NU])
{
	if constexpr (joint_functors<M>::value) {
		M::plantAdjointFunctors(o, x, f, gm, Df, Dg);
	} else {
		M::dynamics(o, x, f, gm);
		M::dynamicsJac(o, x, Df, Dg);
	}
}

// F(X, u) from f and g at X
template <int NX, int NU>
ASIF_HD void plant_closed_loop(const double (&f)[NX], const double (&gm)[NX * NU], const double (&u)[NU], double (&k)[NX])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#pragma unroll
	for (int m = 0; m < NX; m++) {
		double fcl = 0.0;
		fcl += f[m];
#pragma unroll
		for (int j = 0; j < NU; j++) fcl += u[j] * gm[m + j * NX];
		k[m] = fcl;
	}
}

template <int NX>
ASIF_HD void plant_stage_state(const double (&x)[NX], double c, const double (&k)[NX], double (&X)[NX])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#pragma unroll
	for (int m = 0; m < NX; m++) X[m] = x[m] + c * k[m];
}

// x <- x+ under the held input u; f, gm: the model's f and g at x (the values the step's filter was assembled from)
template <class M, int PLANT, class O>
ASIF_HD void plant_step(const O &o, double dt, const double (&f)[M::NX], const double (&gm)[M::NX * M::NU],
                        const double (&u)[M::NU], double (&x)[M::NX])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	constexpr int NX = M::NX, NU = M::NU;
	static_assert(PLANT == kPlantRk4, "the Euler step stays where it has always been written: in the kernel's loop");
	const double hdt = 0.5 * dt, dt6 = dt / 6.0;
	double k1[NX], k2[NX], k3[NX], k4[NX], X[NX], fs[NX], gs[NX * NU];
	plant_closed_loop<NX, NU>(f, gm, u, k1);
	plant_stage_state<NX>(x, hdt, k1, X);
	model_plant_functors<M>(o, X, fs, gs);
	plant_closed_loop<NX, NU>(fs, gs, u, k2);
	plant_stage_state<NX>(x, hdt, k2, X);
	model_plant_functors<M>(o, X, fs, gs);
	plant_closed_loop<NX, NU>(fs, gs, u, k3);
	plant_stage_state<NX>(x, dt, k3, X);
	model_plant_functors<M>(o, X, fs, gs);
	plant_closed_loop<NX, NU>(fs, gs, u, k4);
#pragma unroll
	for (int k = 0; k < NX; k++) x[k] = x[k] + dt6 * (((k1[k] + 2.0 * k2[k]) + 2.0 * k3[k]) + k4[k]);
}

// Xb = J' kb with J = Df + sum_j u_j Dg_j, and gk += g' kb
template <int NX, int NU>
ASIF_HD void plant_stage_adjoint(const double (&gm)[NX * NU], const double (&Df)[NX * NX], const double (&Dg)[NX * NX * NU],
                                 const double (&u)[NU], const double (&kb)[NX], double (&Xb)[NX], double (&gu)[NU])
{
#pragma unroll
	for (int m = 0; m < NX; m++) {
		double t = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) {
			double c = Df[k + m * NX];
#pragma unroll
			for (int j = 0; j < NU; j++) c += u[j] * Dg[k + m * NX + j * NX * NX];
			t += c * kb[k];
		}
		Xb[m] = t;
	}
#pragma unroll
	for (int j = 0; j < NU; j++) {
		double t = 0.0;
#pragma unroll
		for (int k = 0; k < NX; k++) t += gm[k + j * NX] * kb[k];
		gu[j] += t;
	}
}

// The step backwards: mu += dL/du_t through the plant and gul; lamn = dL/dx_t through the plant and gxl (the filter's share
// is the caller's).  f, gm, Df, Dg: the model's at x.
template <class M, int PLANT, class O>
ASIF_HD void plant_step_adjoint(const O &o, double dt, const double (&x)[M::NX], const double (&ut)[M::NU],
                                const double (&f)[M::NX], const double (&gm)[M::NX * M::NU],
                                const double (&Df)[M::NX * M::NX], const double (&Dg)[M::NX * M::NX * M::NU],
                                const double (&lam)[M::NX], const double (&gxl)[M::NX], const double (&gul)[M::NU],
                                double (&mu)[M::NU], double (&lamn)[M::NX])
{
	constexpr int NX = M::NX, NU = M::NU;
	static_assert(PLANT == kPlantRk4, "the Euler adjoint stays where it has always been written: rollout_vjp_step");
	const double hdt = 0.5 * dt, dt6 = dt / 6.0, dt3 = dt / 3.0;
	// the stages again, in the forward pass's order: X2, X3, X4 and the model's f, g, Df, Dg there
	double ks[NX], X[NX];
	double f2[NX], g2[NX * NU], Df2[NX * NX], Dg2[NX * NX * NU];
	double f3[NX], g3[NX * NU], Df3[NX * NX], Dg3[NX * NX * NU];
	double f4[NX], g4[NX * NU], Df4[NX * NX], Dg4[NX * NX * NU];
	plant_closed_loop<NX, NU>(f, gm, ut, ks);
	plant_stage_state<NX>(x, hdt, ks, X);
	model_plant_adjoint_functors<M>(o, X, f2, g2, Df2, Dg2);
	plant_closed_loop<NX, NU>(f2, g2, ut, ks);
	plant_stage_state<NX>(x, hdt, ks, X);
	model_plant_adjoint_functors<M>(o, X, f3, g3, Df3, Dg3);
	plant_closed_loop<NX, NU>(f3, g3, ut, ks);
	plant_stage_state<NX>(x, dt, ks, X);
	model_plant_adjoint_functors<M>(o, X, f4, g4, Df4, Dg4);
	// ... and backwards through them
	double kb[NX], Xb[NX], sum[NX], gu[NU];
#pragma unroll
	for (int j = 0; j < NU; j++) gu[j] = 0.0;
#pragma unroll
	for (int m = 0; m < NX; m++) kb[m] = dt6 * lam[m];
	plant_stage_adjoint<NX, NU>(g4, Df4, Dg4, ut, kb, Xb, gu);
#pragma unroll
	for (int m = 0; m < NX; m++) sum[m] = Xb[m], kb[m] = dt3 * lam[m] + dt * Xb[m];
	plant_stage_adjoint<NX, NU>(g3, Df3, Dg3, ut, kb, Xb, gu);
#pragma unroll
	for (int m = 0; m < NX; m++) sum[m] += Xb[m], kb[m] = dt3 * lam[m] + hdt * Xb[m];
	plant_stage_adjoint<NX, NU>(g2, Df2, Dg2, ut, kb, Xb, gu);
#pragma unroll
	for (int m = 0; m < NX; m++) sum[m] += Xb[m], kb[m] = dt6 * lam[m] + hdt * Xb[m];
	plant_stage_adjoint<NX, NU>(gm, Df, Dg, ut, kb, Xb, gu);
#pragma unroll
	for (int j = 0; j < NU; j++) mu[j] += gul[j] + gu[j];
#pragma unroll
	for (int m = 0; m < NX; m++) lamn[m] = lam[m] + (sum[m] + Xb[m]) + gxl[m];
}

} // namespace asif
