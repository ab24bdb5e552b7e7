// k_explicit_cp.hip -- class ASIF on the synthetic cart-driven pendulum (models.hpp: CartPendulum): the general
// instantiations of the fused explicit filter (explicit_filter.hpp), in a translation unit of their own so that the
// code object of k_explicit.hip -- the double integrator's kernels, the benchmark's among them -- stays what it was.
#include "explicit_filter.hpp"

namespace asif {

// the double integrator's shape (nv = 2, four rows), every solver mode on the general instantiation
int launch_explicit_cp(const DevOptions &o, const asif_hip_solver &S, const FilterArgs &a, bool assemble_only,
                       hipStream_t stream)
{
	if (a.B <= 0) return 0;
	if (S.lanes_per_qp > 1) return ASIF_HIP_EINVAL;
	return launch_g<CartPendulum, 1>(o, S, a, assemble_only, stream);
}

} // namespace asif
