"""Which capi.Filter method the torch rollout functions under a policy call, and when they call none.

No result depends on it where the kernels agree (the params entries with absent parameters compute what the policy entries
compute, the plant entries under Euler what the params entries compute), so the suites that compare results cannot see it.
Double integrator, B = 3 (less than a wave: padded lanes are present), T = 2, K and v given.
"""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, DT = 3, 2, 1e-2
DEV = "cuda:0"


class Recorder:
    """A capi.Filter with every attribute forwarded and the calls of its rollout* methods noted: (name, arguments by
    parameter name, defaults filled in)."""

    def __init__(self, flt):
        self._flt, self.calls = flt, []

    def __getattr__(self, name):
        attr = getattr(self._flt, name)
        if not name.startswith("rollout"):
            return attr

        def noted(*a, **kw):
            bound = inspect.signature(attr).bind(*a, **kw)
            bound.apply_defaults()
            self.calls.append((name, dict(bound.arguments)))
            return attr(*a, **kw)
        return noted

    def names(self):
        return [name for name, _ in self.calls]


class Ctx:
    """What torch hands to forward / backward as ctx, for calling the two directly: a backward pass in which no input
    requires a gradient is not one autograd would start."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad, self.saved_tensors = needs_input_grad, ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


@pytest.fixture(scope="module")
def flt(hip):
    f = hip.Filter(hip.MODEL_DOUBLE_INTEGRATOR, hip.EXPLICIT)
    yield f
    f.close()


def leaves(steps, grad=True):
    t = lambda *shape, at=0.0, step=0.125: (at + step * torch.arange(torch.Size(shape).numel(), dtype=torch.float64)
                                            ).reshape(shape).to(DEV).requires_grad_(grad)
    return dict(x0=t(2, B, at=-0.5), k=t(1, B, at=-0.25), K=t(2, B, at=-0.5), v=t(steps, 1, B, step=0.0625), uprev=t(1, B),
                alpha=t(B, at=1.0), lb=t(1, B, at=-0.75, step=0.0), ub=t(1, B, at=0.75, step=0.0))


def apply(fn, rec, lv, steps, integrator, params):
    """params: None (PolicyRolloutFn), False (ParamRolloutFn, all three None), True (all three given)"""
    head = (rec, lv["x0"], lv["k"], lv["K"], lv["v"], lv["uprev"])
    if params is None:
        return fn.apply(*head, steps, DT, integrator)
    return fn.apply(*head, *((lv["alpha"], lv["lb"], lv["ub"]) if params else (None, None, None)), steps, DT, integrator)


def cases():
    from asif_amd.torch_layer import ParamRolloutFn, PolicyRolloutFn
    return [(PolicyRolloutFn, None, "euler", "rollout_policy"), (PolicyRolloutFn, None, "rk4", "rollout_plant"),
            (ParamRolloutFn, False, "euler", "rollout_params"), (ParamRolloutFn, False, "rk4", "rollout_plant"),
            (ParamRolloutFn, True, "euler", "rollout_params"), (ParamRolloutFn, True, "rk4", "rollout_plant")]


def test_each_case_calls_its_own_entry(hip, flt):
    """One forward and one backward call per case, by name; the plant entries get the integrator, the params and plant
    entries the parameters that were given (and their gradients), the policy function hands none over."""
    for fn, params, integrator, entry in cases():
        rec, lv = Recorder(flt), leaves(T)
        xT, _, _, ulog, _, _ = apply(fn, rec, lv, T, integrator, params)
        (xT.sum() + ulog.sum()).backward()
        torch.cuda.synchronize()
        assert rec.names() == [entry, entry + "_vjp"], (fn.__name__, params, integrator)
        for _, args in rec.calls:
            assert args["T"] == T and args["dt"] == DT
            assert args["K"] is not None and args["v"] is not None
            if entry == "rollout_plant":
                assert args["integrator"] == hip.PLANT_RK4
            if entry != "rollout_policy":
                assert all((args[p] is not None) == bool(params) for p in ("alpha", "lb", "ub"))
        back = rec.calls[1][1]
        assert all(back[g] is not None for g in ("gxT", "gulog", "gK", "gv"))
        assert back["guactT"] is None and back["gxlog"] is None
        if entry != "rollout_policy":
            assert all((back[g] is not None) == bool(params) for g in ("galpha", "glb", "gub"))
        given = ("x0", "k", "K", "v", "uprev") + (("alpha", "lb", "ub") if params else ())
        assert all(lv[name].grad is not None and lv[name].grad.shape == lv[name].shape for name in given)


def test_without_a_step_nothing_runs_forward_and_the_adjoint_gets_no_log(flt):
    """T = 0: no forward call; one backward call, with v, gv and the gradients of the (empty) logs as None."""
    for fn, params, integrator, entry in cases():
        rec, lv = Recorder(flt), leaves(0)
        xT, _, _, ulog, _, _ = apply(fn, rec, lv, 0, integrator, params)
        assert rec.names() == [], (fn.__name__, params, integrator)
        (xT.sum() + ulog.sum()).backward()
        torch.cuda.synchronize()
        assert rec.names() == [entry + "_vjp"], (fn.__name__, params, integrator)
        back = rec.calls[0][1]
        assert back["T"] == 0
        assert all(back[g] is None for g in ("v", "gv", "gxlog", "gulog"))
        assert back["K"] is not None and back["gK"] is not None and back["gxT"] is not None
        assert torch.equal(lv["x0"].grad, torch.ones_like(lv["x0"]))  # the identity
        assert lv["v"].grad is not None and lv["v"].grad.shape == (0, 1, B)


def test_a_backward_pass_nobody_asked_for_makes_no_call(flt):
    """No input requires a gradient, or no output's gradient is given: no call, one None per forward argument."""
    for fn, params, integrator, _ in cases():
        count = 9 if params is None else 12
        for needs, grads in (((False,) * count, True), ((False,) + (True,) * (count - 4) + (False,) * 3, False)):
            rec, lv, ctx = Recorder(flt), leaves(T, grad=False), Ctx(needs)
            head = (rec, lv["x0"], lv["k"], lv["K"], lv["v"], lv["uprev"])
            mid = () if params is None else (lv["alpha"], lv["lb"], lv["ub"]) if params else (None, None, None)
            xT, _, _, ulog, _, _ = fn.forward(ctx, *head, *mid, T, DT, integrator)
            assert len(rec.calls) == 1
            g = (torch.ones_like(xT), None, None, torch.ones_like(ulog), None, None) if grads else (None,) * 6
            assert fn.backward(ctx, *g) == (None,) * count, (fn.__name__, params, integrator, needs)
            assert len(rec.calls) == 1
    torch.cuda.synchronize()
