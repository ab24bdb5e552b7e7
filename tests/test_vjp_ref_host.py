"""The yardstick of tests/test_gpu_explicit_vjp.py, checked without a GPU: the numpy adjoint of tests/vjp_ref.py against
central finite differences of the oracle's exact filter -- no product code involved -- and the new entry's presence in
the header, the binding and the built library."""
import os
import re

import numpy as np
import pytest

import vjp_ref
from asif_amd import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
EPS = 1e-6


def batch(cfg, lie, oracle):
    x, udes = workloads.make_batch(cfg, B)
    d = oracle.dims(*oracle.CONFIGS[cfg], oracle.default_options(*oracle.CONFIGS[cfg]))
    rng = np.random.default_rng(cfg)
    lfh, lgh = rng.normal(0, 1, (d.nc, B)), rng.normal(0, 1, (d.nc * d.nu, B))  # drawn on both paths: same gbar
    gbar = rng.normal(0, 1, (d.nu, B))
    return x, udes, ((lfh, lgh) if lie else None), gbar


def _loss(oracle, cfg, x, udes, lie, gbar):
    ua, rc = vjp_ref.solve(oracle, cfg, np.ascontiguousarray(x.T), np.ascontiguousarray(udes.T), lie)
    return (ua.T * gbar).sum(axis=0), rc  # one scalar per instance: instances are independent


def _fd(oracle, cfg, x, udes, lie, gbar, which, comp):
    """Central difference of every instance's loss in component `comp` of input `which`, all instances at once."""
    vals = []
    for s in (+1.0, -1.0):
        xx, uu, ll = x.copy(), udes.copy(), (None if lie is None else (lie[0].copy(), lie[1].copy()))
        {"x": xx, "udes": uu, "lfh": ll and ll[0], "lgh": ll and ll[1]}[which][comp] += s * EPS
        vals.append(_loss(oracle, cfg, xx, uu, ll, gbar))
    same = (vals[0][1] == 1) & (vals[1][1] == 1)
    return (vals[0][0] - vals[1][0]) / (2 * EPS), same


@pytest.mark.parametrize("cfg,lie", [(2, False), (2, True), (11, False), (11, True)])
def test_numpy_adjoint_matches_finite_differences_of_the_oracle(oracle, cfg, lie):
    """Bounds, per gradient entry, relative to 1 + |reference|:

    udes: u* is piecewise LINEAR in uDes, so the central difference has no truncation error and must agree to
    rounding: two exact optima, each good to a few ulps of |u*| <= 1.5, times |gbar| <= 4.5, over 2 eps = 2e-6 -- a
    dozen ulps come to 1e-8, the bound.  Measured maximum 2.2e-10.
    lfh, lgh, x: u* is linear in Lfh as well, rational in Lgh, and h is quadratic in x on the double integrator's
    braking rows (a truncation term of order eps^2 on top of the rounding).  Measured maxima over these four batches:
    lfh 1.7e-10, lgh 8.3e-10, x 1.6e-10; each is asserted at 10 x its measured maximum.
    """
    x, udes, lies, gbar = batch(cfg, lie, oracle)
    ref = vjp_ref.vjp(oracle, cfg, x, udes, gbar, lies)
    good = (ref["rc"] == 1) & ~ref["degenerate"]
    assert good.sum() >= 0.99 * (ref["rc"] == 1).sum() and good.sum() > 1000
    assert (ref["rc"] == -1).sum() > 400
    nc, nu, nx = ref["glfh"].shape[0], ref["gudes"].shape[0], ref["gx"].shape[0]
    plan = [("udes", "gudes", nu, 1e-8)]
    if lie:
        plan += [("lfh", "glfh", nc, 1.7e-9), ("lgh", "glgh", nc * nu, 8.3e-9), ("x", "gx", nx, 1.6e-9)]
    for which, key, n, tol in plan:
        worst = 0.0
        for comp in range(n):
            fd, same = _fd(oracle, cfg, x, udes, lies, gbar, which, comp)
            m = good & same
            assert m.sum() >= good.sum() - 2  # a perturbed instance may leave the feasible set; not the rule
            gap = np.abs(fd[m] - ref[key][comp][m]) / (1.0 + np.abs(ref[key][comp][m]))
            worst = max(worst, float(gap.max()))
        print(f"cfg {cfg} lie={lie} d/d{which}: max gap {worst:.3e} (bound {tol:.1e})")
        assert worst <= tol, (which, worst)


def test_reference_flags_what_it_should(oracle):
    """The degenerate flag and the working-set census on the cfg 11 batches: every class of working-set size is there."""
    for lie in (False, True):
        x, udes, lies, gbar = batch(11, lie, oracle)
        ref = vjp_ref.vjp(oracle, 11, x, udes, gbar, lies)
        ok = ref["rc"] == 1
        assert {0, 1, 2} <= set(ref["nactive"][ok & ~ref["degenerate"]])
        assert ref["degenerate"][ok].mean() <= 0.01
        assert np.all(ref["gudes"][:, ~ok] == 0.0)


def test_vjp_entry_is_declared_bound_and_exported():
    name = "asif_hip_filter_vjp_batch"
    header = open(os.path.join(ROOT, "include", "asif_hip.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), "not declared in include/asif_hip.h"
    assert int(re.search(r"#define ASIF_HIP_VERSION (\d+)", header).group(1)) >= 140
    from asif_amd import capi
    assert name in capi.EXPORTS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load()
    assert hasattr(lib, name)
    assert lib.asif_hip_version() >= 140
    assert hasattr(capi.Filter, "filter_vjp")
