#!/usr/bin/env python3
"""Times the parameter rollout's two entries against the policy entries on cuda:0.

    python tools/time_rollout_params.py [--parent-lib PATH] [--B 65536] [--T 100] [--reps 200] [--out FILE]

Every variant is one launch between two device events; the variants alternate inside each repetition, so they share
whatever else the machine is doing; x / uact / relax are restored before every forward launch, outside the timed window.
Per variant: median, 10th and 90th percentile over the repetitions (after a warm-up), in microseconds, and the ratio of
the medians to the baseline.  --parent-lib: a libasif_hip.so built from the parent commit, whose
asif_hip_rollout_policy_batch / asif_hip_rollout_policy_vjp_batch (with K and v) serve as the baseline; without it the
baseline is this tree's own.  The new entries run with K and v too: without parameters, with alpha alone, and with all
three parameters (backward: all three gradients).  All logs are written (forward) and all incoming gradients given
(backward); every backward variant sweeps the logs of its own forward pass.  Prints one JSON object; --out also writes it.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asif_amd import capi, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    B, T, dt = a.B, a.T, a.dt

    new = capi.load()
    base = new
    if a.parent_lib:
        base = C.CDLL(a.parent_lib)
        for name in ("asif_hip_create", "asif_hip_destroy", "asif_hip_rollout_policy_batch",
                     "asif_hip_rollout_policy_vjp_batch"):
            getattr(base, name).argtypes = getattr(new, name).argtypes

    def handle(lib):
        h = C.c_void_p()
        o, s = capi.default_options(capi.MODEL_DOUBLE_INTEGRATOR, capi.EXPLICIT), capi.default_solver()
        capi.check(lib.asif_hip_create(C.byref(h), capi.MODEL_DOUBLE_INTEGRATOR, capi.EXPLICIT, C.byref(o), C.byref(s), 0))
        return h
    hn, hb = handle(new), handle(base)

    x0n, kn = workloads.make_batch(2, B)
    rng = np.random.default_rng(1)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    x0, k = t(x0n), t(kn)
    K = t(np.array([[-2.0], [-3.0]]) + 0.5 * rng.normal(0, 1, (2, B)))
    v = t(0.3 * rng.normal(0, 1, (T, 1, B)))
    i = np.arange(B, dtype=np.uint64)
    alpha = t(2.0 + 6.0 * workloads.uniform(480, i, 0))
    lb, ub = t((-1.5 + workloads.uniform(480, i, 1))[None, :]), t((0.5 + workloads.uniform(480, i, 2))[None, :])
    u0 = z(1, B)
    x, uact, relax, nfail = z(2, B), z(1, B), z(1, B), z(B, dtype=torch.int32)
    p = lambda tt: None if tt is None else C.c_void_p(tt.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def logs():
        return z(T, 2, B), z(T, 1, B), z(T, B, dtype=torch.int32)

    def restore():
        x.copy_(x0)
        uact.copy_(u0)
        relax.zero_()

    def fwd_policy(lg):
        return lambda: base.asif_hip_rollout_policy_batch(hb, B, B, T, dt, p(x), p(K), p(k), p(v), p(uact), p(relax),
                                                          p(nfail), p(lg[0]), p(lg[1]), p(lg[2]), stream())

    def fwd_params(lg, al, lo, hi):
        return lambda: new.asif_hip_rollout_params_batch(hn, B, B, T, dt, p(x), p(K), p(k), p(v), p(al), p(lo), p(hi),
                                                         p(uact), p(relax), p(nfail), p(lg[0]), p(lg[1]), p(lg[2]), stream())

    sets = {"null": (None, None, None), "alpha": (alpha, None, None), "full": (alpha, lb, ub)}
    lg_base, lg = logs(), {name: logs() for name in sets}
    restore()
    capi.check(fwd_policy(lg_base)())
    for name, par in sets.items():
        restore()
        capi.check(fwd_params(lg[name], *par)())
    torch.cuda.synchronize()
    gxT, guT = t(rng.normal(0, 1, (2, B))), t(rng.normal(0, 1, (1, B)))
    gxl, gul = t(rng.normal(0, 1, (T, 2, B))), t(rng.normal(0, 1, (T, 1, B)))
    gx0, gk, gu0, gK, gv, nskip = z(2, B), z(1, B), z(1, B), z(2, B), z(T, 1, B), z(B, dtype=torch.int32)
    ga, gl, gu = z(B), z(1, B), z(1, B)

    def bwd_policy():
        l = lg_base
        return base.asif_hip_rollout_policy_vjp_batch(hb, B, B, T, dt, p(l[0]), p(l[1]), p(l[2]), p(K), p(k), p(v), p(gxT),
                                                      p(guT), p(gxl), p(gul), p(gx0), p(gK), p(gk), p(gv), p(gu0), p(nskip),
                                                      stream())

    def bwd_params(l, par, gpar):
        return lambda: new.asif_hip_rollout_params_vjp_batch(hn, B, B, T, dt, p(l[0]), p(l[1]), p(l[2]), p(K), p(k), p(v),
                                                             *[p(q) for q in par], p(gxT), p(guT), p(gxl), p(gul), p(gx0),
                                                             p(gK), p(gk), p(gv), *[p(q) for q in gpar], p(gu0), p(nskip),
                                                             stream())

    scratch = logs()  # timed forward launches write here: the logs above stay the backward passes' inputs
    variants = [("forward_policy_baseline", fwd_policy(scratch), True),
                ("forward_params_null", fwd_params(scratch, *sets["null"]), True),
                ("forward_params_alpha", fwd_params(scratch, *sets["alpha"]), True),
                ("forward_params_full", fwd_params(scratch, *sets["full"]), True),
                ("backward_policy_baseline", bwd_policy, False),
                ("backward_params_null", bwd_params(lg["null"], sets["null"], (None, None, None)), False),
                ("backward_params_alpha", bwd_params(lg["alpha"], sets["alpha"], (ga, None, None)), False),
                ("backward_params_full", bwd_params(lg["full"], sets["full"], (ga, gl, gu)), False)]
    times = {name: [] for name, _, _ in variants}
    for rep in range(a.warmup + a.reps):
        for name, call, is_fwd in variants:
            if is_fwd:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.check(call())
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = dict(B=B, T=T, dt=dt, reps=a.reps, baseline="parent library" if a.parent_lib else "this tree", us={})
    for name, ts in times.items():
        q = np.percentile(ts, [10, 50, 90])
        res["us"][name] = dict(median=round(float(q[1]), 2), p10=round(float(q[0]), 2), p90=round(float(q[2]), 2))
    med = lambda n: res["us"][n]["median"]
    res["ratio_to_baseline"] = {n: round(med(n) / med(n.split("_")[0] + "_policy_baseline"), 3) for n in times}
    assert int(nskip.max()) == 0
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    new.asif_hip_destroy(hn)
    base.asif_hip_destroy(hb)


if __name__ == "__main__":
    main()
