// rollout_policy_step.hpp -- the fused explicit rollout under an affine policy, per instance and in registers: the
// policy's one evaluation order, and one step of the adjoint.
//
// Forward step t on the state x_t the filter sees (k_rollout_policy.hip: rollout_policy_kernel):
//     uDes_t = k + K x_t + v_t;   (ok_t, u*_t) = filter(x_t, uDes_t);   u_t = ok_t ? u*_t : u_{t-1};
//     x_{t+1} = x_t + dt (f(x_t) + g(x_t) u_t)
// K [nu x nx], entry (j, m) at j + m nu, and v_t are each optional: an absent term is not evaluated at all.
// policy_udes is the only place uDes_t is formed -- by the forward kernel, by the backward kernel (which recomputes it
// from the logged x_t and must get the forward pass's bits) and by the host driver of the tests: start from k_j, add
// K[j,m] x_m for m = 0 ... nx-1, then add v_t,j, no contraction.
//
// Backward step: rollout_vjp_step.hpp unchanged, called with its gudes zeroed, so that what it leaves there is the
// step's own d_t = dL/duDes_t (mu on a free step; zero on a failed step and on one that ends on a row or a bound), and
//     gk += d_t;   gK[j,m] += d_t[j] x_t[m];   gv[t] = d_t (the caller's store);   lambda += K' d_t
// where lambda is the value the step leaves for t-1: x_t reaches uDes_t through K.  out is the wrapped step's, passed on.
//
// Compiles for the host like the file it wraps (tests/host_rollout_policy_driver.cpp).
#pragma once
#include "rollout_vjp_step.hpp"

namespace asif {

template <int NX, int NU>
ASIF_HD void policy_udes(const double (&k)[NU], const double (&K)[NU * NX], bool hasK, const double (&x)[NX],
                         const double (&v)[NU], bool hasV, double (&uDes)[NU])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#pragma unroll
	for (int j = 0; j < NU; j++) {
		double a = k[j];
		if (hasK) { // the same for every instance of a launch
#pragma unroll
			for (int m = 0; m < NX; m++) a = a + K[j + m * NU] * x[m];
		}
		if (hasV) a = a + v[j];
		uDes[j] = a;
	}
}

template <class M>
struct PolicyAdjoint { // what the policy sweep carries from step to step
	RolloutAdjoint<M> s; // s.gudes holds the last step's d_t
	double gk[M::NU], gK[M::NU * M::NX];
};

template <class M, int PLANT = kPlantEuler, class O>
ASIF_HD void rollout_policy_vjp_step(const O &o, const RolloutVjpOpts<M::NU> &e, double dt, const double (&x)[M::NX],
                                     const double (&ut)[M::NU], const double (&k)[M::NU],
                                     const double (&K)[M::NU * M::NX], bool hasK, const double (&v)[M::NU], bool hasV,
                                     int rc, const double (&gxl)[M::NX], const double (&gul)[M::NU], PolicyAdjoint<M> &p,
                                     StepWorkingSet<M> *out = nullptr)
{
	constexpr int NX = M::NX, NU = M::NU;
	double uDes[NU];
	policy_udes<NX, NU>(k, K, hasK, x, v, hasV, uDes);
#pragma unroll
	for (int j = 0; j < NU; j++) p.s.gudes[j] = 0.0;
	rollout_vjp_step<M, PLANT>(o, e, dt, x, ut, uDes, rc, gxl, gul, p.s, out);
#pragma unroll
	for (int j = 0; j < NU; j++) p.gk[j] += p.s.gudes[j];
	if (hasK) {
#pragma unroll
		for (int m = 0; m < NX; m++) {
			double t = 0.0;
#pragma unroll
			for (int j = 0; j < NU; j++) {
				p.gK[j + m * NU] += p.s.gudes[j] * x[m];
				t += K[j + m * NU] * p.s.gudes[j];
			}
			p.s.lam[m] += t;
		}
	}
}

} // namespace asif
