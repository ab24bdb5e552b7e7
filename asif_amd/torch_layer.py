"""Differentiable torch layers on the library's kernels.

The explicit safety filter (class ASIF).  Forward: asif_hip_filter_batch / asif_hip_filter_batch_lie.  Backward: one
asif_hip_filter_vjp_batch launch (asif_amd/csrc/k_explicit_vjp.hip).
The fused explicit rollout, T x (filter + plant Euler step) on the double integrator.  Forward: asif_hip_rollout_batch.
Backward: one asif_hip_rollout_vjp_batch launch (asif_amd/csrc/k_rollout_vjp.hip), state gradient included.
The same rollout under an affine policy udes_t = k + K x_t + v_t evaluated inside the loop, on the double integrator or
the cart-driven pendulum (capi.MODEL_CART_PENDULUM, a nonlinear plant), optionally with the barrier gain and the input box
per instance.  Forward: asif_hip_rollout_policy_batch / asif_hip_rollout_params_batch.  Backward: one
asif_hip_rollout_policy_vjp_batch / asif_hip_rollout_params_vjp_batch launch (asif_amd/csrc/k_rollout_policy.hip).
The batched solve of small pre-assembled QPs.  Forward: asif_hip_qp_solve_batch.  Backward: one asif_hip_qp_vjp_batch
launch (asif_amd/csrc/k_qp_vjp.hip).
All of it runs on torch's current stream; nothing here computes on the CPU, and no solve or adjoint falls back to torch
operators.  The torch operators that remain are bookkeeping around the launches: an instance whose forward pass failed
has its incoming gradient routed (ExplicitFilterFn: to uact_prev) or zeroed (QPSolveFn) by one elementwise select.

Tensors are FP64 CUDA tensors, structure-of-arrays: x [nx,B], udes [nu,B], lfh [nc,B], lgh [nc*nu,B]; for the QP
Hd, c, lb, ub [nv,B], A [nc*nv,B] (entry (r, j) of the row matrix at component r + j*nc), b [nc,B].
"""
import torch

from . import capi


# the models the fused rollouts under a policy (PolicyRolloutFn, ParamRolloutFn) are compiled for
ROLLOUT_MODELS = (capi.MODEL_DOUBLE_INTEGRATOR, capi.MODEL_CART_PENDULUM)


def _soa(t, rows, B, name):
    if t.dtype != torch.float64 or not t.is_cuda or t.shape != (rows, B):
        raise ValueError(f"{name}: expected a float64 CUDA tensor of shape ({rows}, {B}), got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t.detach().contiguous()


class ExplicitFilterFn(torch.autograd.Function):
    """uact, rc = ExplicitFilterFn.apply(flt, x, udes, lfh, lgh, uact_prev)

    flt: an explicit capi.Filter.  lfh / lgh: both tensors (caller-supplied Lie derivatives) or both None (the model's
    own).  uact_prev [nu,B] or None (zeros): what uact holds where the QP fails (rc < 0), as ASIF::filter leaves it.
    Gradients flow to udes, uact_prev and, on the caller-supplied path, to lfh, lgh and x (through h alone: the caller's
    graph carries the part through lfh and lgh).  On the model path x takes no gradient: that would need the model's
    second derivatives, and asking for it is an error.  rc is not differentiable."""

    @staticmethod
    def forward(ctx, flt, x, udes, lfh, lgh, uact_prev):
        d = flt.dims
        B = x.shape[1]
        if (lfh is None) != (lgh is None):
            raise ValueError("lfh and lgh are given together or not at all")
        lie = lfh is not None
        if not lie and ctx.needs_input_grad[1]:
            raise RuntimeError("x requires grad, but with the model's own Lie derivatives the filter has no gradient "
                               "with respect to x (it would need the model's second derivatives): detach x, or supply "
                               "lfh and lgh from a differentiable model")
        x, udes = _soa(x, d.nx, B, "x"), _soa(udes, d.nu, B, "udes")
        if lie:
            lfh, lgh = _soa(lfh, d.nc, B, "lfh"), _soa(lgh, d.nc * d.nu, B, "lgh")
        uact = (_soa(uact_prev, d.nu, B, "uact_prev").clone() if uact_prev is not None
                else torch.zeros((d.nu, B), dtype=torch.float64, device=x.device))
        relax = torch.zeros((d.nrelax, B), dtype=torch.float64, device=x.device)
        rc = torch.zeros(B, dtype=torch.int32, device=x.device)
        if B > 0:
            if lie:
                flt.filter_lie(x, udes, lfh, lgh, uact, relax, rc)
            else:
                flt.filter(x, udes, uact, relax, rc)
        ctx.flt, ctx.lie = flt, lie
        ctx.save_for_backward(x, udes, rc, *((lfh, lgh) if lie else ()))
        ctx.mark_non_differentiable(rc)
        return uact, rc

    @staticmethod
    def backward(ctx, guact, _grc):
        x, udes, rc = ctx.saved_tensors[:3]
        lfh, lgh = ctx.saved_tensors[3:] if ctx.lie else (None, None)
        guact = guact.contiguous()
        gudes = torch.empty_like(udes)
        glfh = torch.empty_like(lfh) if ctx.lie and ctx.needs_input_grad[3] else None
        glgh = torch.empty_like(lgh) if ctx.lie and ctx.needs_input_grad[4] else None
        gx = torch.empty_like(x) if ctx.lie and ctx.needs_input_grad[1] else None
        if x.shape[1] > 0:
            ctx.flt.filter_vjp(x, udes, guact, gudes, torch.empty_like(rc), lfh, lgh, glfh, glgh, gx)
        # a failed instance kept uact_prev: its dL/duAct belongs there
        gprev = torch.where(rc < 0, guact, torch.zeros_like(guact)) if ctx.needs_input_grad[5] else None
        return None, gx, gudes, glfh, glgh, gprev


class ExplicitSafetyLayer(torch.nn.Module):
    """Owns an explicit capi.Filter (class ASIF on `model`) and applies it as the last layer of a policy:
    uact, rc = layer(x, udes[, lfh, lgh][, uact_prev=...])."""

    def __init__(self, model=capi.MODEL_DOUBLE_INTEGRATOR, options=None, solver=None, device=0):
        super().__init__()
        self.filter = capi.Filter(model, capi.EXPLICIT, options=options, solver=solver, device=device)

    def forward(self, x, udes, lfh=None, lgh=None, uact_prev=None):
        return ExplicitFilterFn.apply(self.filter, x, udes, lfh, lgh, uact_prev)


def _rollout_buffers(d, B, T, uact_prev, device):
    """What a T-step rollout writes: uact (a copy of uact_prev, or zeros), relax, nfail and the logs xlog, ulog, rclog."""
    uact = (_soa(uact_prev, d.nu, B, "uact_prev").clone() if uact_prev is not None
            else torch.zeros((d.nu, B), dtype=torch.float64, device=device))
    relax = torch.zeros((d.nrelax, B), dtype=torch.float64, device=device)
    nfail = torch.zeros(B, dtype=torch.int32, device=device)
    xlog = torch.zeros((T, d.nx, B), dtype=torch.float64, device=device)
    ulog = torch.zeros((T, d.nu, B), dtype=torch.float64, device=device)
    rclog = torch.zeros((T, B), dtype=torch.int32, device=device)
    return uact, relax, nfail, xlog, ulog, rclog


class ExplicitRolloutFn(torch.autograd.Function):
    """xT, uactT, xlog, ulog, rclog, nfail = ExplicitRolloutFn.apply(flt, x0, udes, uact_prev, T, dt)

    T closed-loop steps of class ASIF on the double integrator (flt: an explicit capi.Filter on that model) with udes
    held: what a policy running at a lower rate than the filter sees between two of its calls.  uact_prev [nu,B] or None
    (zeros, no gradient): the input applied where the first filter call fails.  xlog [T,nx,B] holds the state each call
    saw, ulog [T,nu,B] the input applied after it; rclog int32 [T,B] and nfail int32 [B] are not differentiable.
    Gradients flow to x0, udes and uact_prev from xT, uactT, xlog and ulog.  Forward is one asif_hip_rollout_batch launch
    with all three logs, backward one asif_hip_rollout_vjp_batch launch on them; gradients of outputs the caller did not
    use are handed to it as NULL.  To change udes along a trajectory -- state feedback, a planned input sequence -- use
    PolicyRolloutFn / PolicyRolloutLayer: the same rollout with udes_t = k + K x_t + v_t evaluated inside the launch."""

    @staticmethod
    def forward(ctx, flt, x0, udes, uact_prev, T, dt):
        d = flt.dims
        B = x0.shape[1]
        T = int(T)
        if T < 0:
            raise ValueError(f"T: expected a non-negative step count, got {T}")
        if flt.model != capi.MODEL_DOUBLE_INTEGRATOR or flt.variant != capi.EXPLICIT:
            raise ValueError("the differentiable rollout with udes held exists for the explicit filter on the double "
                             "integrator only; on the cart-driven pendulum use PolicyRolloutFn with K = v = None")
        x = _soa(x0, d.nx, B, "x0").clone()
        udes = _soa(udes, d.nu, B, "udes")
        uact, relax, nfail, xlog, ulog, rclog = _rollout_buffers(d, B, T, uact_prev, x.device)
        if B > 0 and T > 0:
            flt.rollout(T, float(dt), x, udes, uact, relax, nfail, xlog, ulog, rclog)
        ctx.flt, ctx.T, ctx.dt = flt, T, float(dt)
        ctx.save_for_backward(xlog, ulog, rclog, udes)
        ctx.mark_non_differentiable(rclog, nfail)
        ctx.set_materialize_grads(False)
        return x, uact, xlog, ulog, rclog, nfail

    @staticmethod
    def backward(ctx, gxT, guactT, gxlog, gulog, _grclog, _gnfail):
        xlog, ulog, rclog, udes = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        given = [g for g in (gxT, guactT, gxlog, gulog) if g is not None]
        if not any(need) or not given:  # nothing asked for, or no output was used: nothing to launch
            return None, None, None, None, None, None
        d = ctx.flt.dims
        B = udes.shape[1]
        cont = lambda g: None if g is None else g.contiguous()
        gxT = cont(gxT) if gxT is not None else torch.zeros((d.nx, B), dtype=torch.float64, device=udes.device)
        gx0 = torch.empty((d.nx, B), dtype=torch.float64, device=udes.device)
        gudes, guact0 = torch.empty_like(udes), torch.empty_like(udes)
        if B > 0:
            ctx.flt.rollout_vjp(ctx.T, ctx.dt, xlog, ulog, rclog, udes, gxT, gx0, gudes, guact0,
                                torch.empty(B, dtype=torch.int32, device=udes.device), guactT=cont(guactT),
                                gxlog=cont(gxlog) if ctx.T > 0 else None, gulog=cont(gulog) if ctx.T > 0 else None)
        return (None, gx0 if need[0] else None, gudes if need[1] else None, guact0 if need[2] else None, None, None)


class ExplicitRolloutLayer(torch.nn.Module):
    """Owns an explicit capi.Filter and rolls the closed loop out for T steps of dt with udes held:
    xT, uactT, xlog, ulog, rclog, nfail = layer(x0, udes[, uact_prev])."""

    def __init__(self, model=capi.MODEL_DOUBLE_INTEGRATOR, options=None, solver=None, device=0, T=1, dt=1e-3):
        super().__init__()
        self.filter = capi.Filter(model, capi.EXPLICIT, options=options, solver=solver, device=device)
        self.T, self.dt = int(T), float(dt)

    def forward(self, x0, udes, uact_prev=None):
        return ExplicitRolloutFn.apply(self.filter, x0, udes, uact_prev, self.T, self.dt)


def _plant(integrator):
    """"euler" / "rk4" -> capi.PLANT_EULER / capi.PLANT_RK4."""
    try:
        return {"euler": capi.PLANT_EULER, "rk4": capi.PLANT_RK4}[integrator]
    except (KeyError, TypeError):
        raise ValueError(f'integrator: expected "euler" or "rk4", got {integrator!r}') from None


def _policy_rollout_entry(plant, has_params):
    """The capi.Filter method of the forward pass; its adjoint is the same name with _vjp."""
    if plant != capi.PLANT_EULER:
        return "rollout_plant"
    return "rollout_params" if has_params else "rollout_policy"


def _policy_rollout_forward(ctx, flt, x0, k, K, v, uact_prev, params, T, dt, integrator):
    """PolicyRolloutFn.forward (params None) and ParamRolloutFn.forward (params = (alpha, lb, ub), each may be None)."""
    plant = _plant(integrator)
    d = flt.dims
    B = x0.shape[1]
    T = int(T)
    if T < 0:
        raise ValueError(f"T: expected a non-negative step count, got {T}")
    if flt.model not in ROLLOUT_MODELS or flt.variant != capi.EXPLICIT:
        raise ValueError("the differentiable rollout under a policy exists for the explicit filter on the double "
                         "integrator and on the cart-driven pendulum")
    x = _soa(x0, d.nx, B, "x0").clone()
    k = _soa(k, d.nu, B, "k")
    K = _soa(K, d.nu * d.nx, B, "K") if K is not None else None
    if v is not None:
        if v.dim() != 3 or v.shape[0] != T:
            raise ValueError(f"v: expected shape ({T}, {d.nu}, {B}), got {tuple(v.shape)}")
        v = _soa(v.reshape(T * d.nu, B), T * d.nu, B, "v").reshape(T, d.nu, B)
    opt = dict(K=K, v=v)
    if params is not None:
        alpha, lb, ub = params
        if alpha is not None:
            if alpha.dim() != 1:
                raise ValueError(f"alpha: expected shape ({B},), got {tuple(alpha.shape)}")
            alpha = _soa(alpha[None, :], 1, B, "alpha")[0]
        lb = _soa(lb, d.nu, B, "lb") if lb is not None else None
        ub = _soa(ub, d.nu, B, "ub") if ub is not None else None
        opt.update(alpha=alpha, lb=lb, ub=ub)
    uact, relax, nfail, xlog, ulog, rclog = _rollout_buffers(d, B, T, uact_prev, x.device)
    if B > 0 and T > 0:
        getattr(flt, _policy_rollout_entry(plant, params is not None))(
            T, float(dt), *(() if plant == capi.PLANT_EULER else (plant,)), x, k, uact, relax, nfail, **opt, xlog=xlog,
            ulog=ulog, rclog=rclog)
    ctx.flt, ctx.T, ctx.dt, ctx.plant, ctx.params = flt, T, float(dt), plant, params is not None
    ctx.opt = tuple(name for name, t in opt.items() if t is not None)
    ctx.save_for_backward(xlog, ulog, rclog, k, *(opt[name] for name in ctx.opt))
    ctx.mark_non_differentiable(rclog, nfail)
    ctx.set_materialize_grads(False)
    return x, uact, xlog, ulog, rclog, nfail


def _policy_rollout_backward(ctx, gxT, guactT, gxlog, gulog):
    """The backward pass of both: one gradient per forward argument, the optional integrator included (autograd drops it
    where it was not passed) -- 9 without the parameters, 12 with them."""
    xlog, ulog, rclog, k = ctx.saved_tensors[:4]
    opt = dict(zip(ctx.opt, ctx.saved_tensors[4:]))
    K, v = opt.get("K"), opt.get("v")
    pnames = ("alpha", "lb", "ub") if ctx.params else ()
    need = ctx.needs_input_grad[1:6 + len(pnames)]  # x0, k, K, v, uact_prev[, alpha, lb, ub]
    given = [g for g in (gxT, guactT, gxlog, gulog) if g is not None]
    if not any(need) or not given:  # nothing asked for, or no output was used: nothing to launch
        return (None,) * (9 + len(pnames))
    d = ctx.flt.dims
    B, T = k.shape[1], ctx.T
    cont = lambda g: None if g is None else g.contiguous()
    gxT = cont(gxT) if gxT is not None else torch.zeros((d.nx, B), dtype=torch.float64, device=k.device)
    gx0 = torch.empty((d.nx, B), dtype=torch.float64, device=k.device)
    gk, guact0 = torch.empty_like(k), torch.empty_like(k)
    gK = torch.empty_like(K) if K is not None and need[2] else None
    gv = torch.empty_like(v) if v is not None and need[3] else None
    # galpha / glb / gub: only for a parameter that was given and requires a gradient
    pgrad = {"g" + name: torch.empty_like(opt[name]) if name in opt and nd else None for name, nd in zip(pnames, need[5:])}
    if B > 0:
        steps = T > 0  # without a step there is no log, no v and no gv to hand over
        getattr(ctx.flt, _policy_rollout_entry(ctx.plant, ctx.params) + "_vjp")(
            T, ctx.dt, *(() if ctx.plant == capi.PLANT_EULER else (ctx.plant,)), xlog, ulog, rclog, k, gxT, gx0, gk, guact0,
            torch.empty(B, dtype=torch.int32, device=k.device), K=K, v=v if steps else None,
            **{name: opt.get(name) for name in pnames}, guactT=cont(guactT), gxlog=cont(gxlog) if steps else None,
            gulog=cont(gulog) if steps else None, gK=gK, gv=gv if steps else None, **pgrad)
    return (None, gx0 if need[0] else None, gk if need[1] else None, gK, gv, guact0 if need[4] else None,
            *pgrad.values(), None, None, None)


class PolicyRolloutFn(torch.autograd.Function):
    """xT, uactT, xlog, ulog, rclog, nfail = PolicyRolloutFn.apply(flt, x0, k, K, v, uact_prev, T, dt[, integrator])

    ExplicitRolloutFn with the desired input coming from an affine policy evaluated inside the loop, on the double
    integrator or the cart-driven pendulum (flt: an explicit capi.Filter on one of ROLLOUT_MODELS):
    udes_t = k + K x_t + v_t.  k [nu,B]; K [nu*nx,B] (entry (j, m) of an instance's gain at component j + m*nu) or None;
    v [T,nu,B] (a planned input sequence) or None; an absent term is not evaluated.  uact_prev and the outputs as
    ExplicitRolloutFn.  Gradients flow to x0, k, K, v and uact_prev from xT, uactT, xlog and ulog.  Forward is one
    asif_hip_rollout_policy_batch launch with all three logs, backward one asif_hip_rollout_policy_vjp_batch launch on
    them; gradients of outputs the caller did not use are handed to it as NULL, and gK / gv are asked for only where K / v
    require a gradient.  A gain shared by the batch is K.expand(-1, B) of a [nu*nx,1] parameter: autograd's own sum over
    the expanded axis turns the per-instance gK into the shared gain's gradient (likewise k and v).
    The policy's output is not returned: udes_t = k + K xlog[t] + v[t] in torch, and gxlog carries its state part back.
    integrator: "euler" (the default: the launches above) or "rk4", the plant stepped by a fourth-order Runge-Kutta step
    with u_t held over dt, forward and backward through asif_hip_rollout_plant_batch / _vjp_batch.  Those are the
    params entries' kernels: under "rk4" this function runs them with alpha = lb = ub = NULL (the handle's values in every
    lane), which computes what a policy kernel would.  The filter is evaluated at the sample instants only under either."""

    @staticmethod
    def forward(ctx, flt, x0, k, K, v, uact_prev, T, dt, integrator="euler"):
        return _policy_rollout_forward(ctx, flt, x0, k, K, v, uact_prev, None, T, dt, integrator)

    @staticmethod
    def backward(ctx, gxT, guactT, gxlog, gulog, _grclog, _gnfail):
        return _policy_rollout_backward(ctx, gxT, guactT, gxlog, gulog)


class ParamRolloutFn(torch.autograd.Function):
    """xT, uactT, xlog, ulog, rclog, nfail = ParamRolloutFn.apply(flt, x0, k, K, v, uact_prev, alpha, lb, ub, T, dt
                                                                  [, integrator])

    PolicyRolloutFn with the filter's own parameters per instance: alpha [B], the barrier gain of
    Lgh u + alpha h >= -Lfh (options.relaxLb), and the input box lb, ub [nu,B]; None is the handle's value.  Gradients
    flow to x0, k, K, v, uact_prev, alpha, lb and ub.  Forward is one asif_hip_rollout_params_batch launch, backward one
    asif_hip_rollout_params_vjp_batch launch; galpha / glb / gub are asked for only where the tensor requires a gradient.
    A gain shared by the batch is alpha.expand(B) of a one-element parameter: autograd's own sum over the expanded axis
    turns the per-instance galpha into the shared gain's gradient (likewise lb and ub through expand(-1, B)).
    integrator: as PolicyRolloutFn's; "rk4" runs asif_hip_rollout_plant_batch / _vjp_batch."""

    @staticmethod
    def forward(ctx, flt, x0, k, K, v, uact_prev, alpha, lb, ub, T, dt, integrator="euler"):
        return _policy_rollout_forward(ctx, flt, x0, k, K, v, uact_prev, (alpha, lb, ub), T, dt, integrator)

    @staticmethod
    def backward(ctx, gxT, guactT, gxlog, gulog, _grclog, _gnfail):
        return _policy_rollout_backward(ctx, gxT, guactT, gxlog, gulog)


class _PolicyRolloutLayer(torch.nn.Module):
    """Owns an explicit capi.Filter and the rollout's T, dt and integrator."""

    def __init__(self, model=capi.MODEL_DOUBLE_INTEGRATOR, options=None, solver=None, device=0, T=1, dt=1e-3,
                 integrator="euler"):
        super().__init__()
        _plant(integrator)
        self.filter = capi.Filter(model, capi.EXPLICIT, options=options, solver=solver, device=device)
        self.T, self.dt, self.integrator = int(T), float(dt), integrator


class PolicyRolloutLayer(_PolicyRolloutLayer):
    """Owns an explicit capi.Filter and rolls the closed loop out for T steps of dt under udes_t = k + K x_t + v_t:
    xT, uactT, xlog, ulog, rclog, nfail = layer(x0, k, K=None, v=None, uact_prev=None)."""

    def forward(self, x0, k, K=None, v=None, uact_prev=None):
        return PolicyRolloutFn.apply(self.filter, x0, k, K, v, uact_prev, self.T, self.dt, self.integrator)


class ParamRolloutLayer(_PolicyRolloutLayer):
    """Owns an explicit capi.Filter and rolls the closed loop out for T steps of dt under udes_t = k + K x_t + v_t with
    the barrier gain and the input box per instance:
    xT, uactT, xlog, ulog, rclog, nfail = layer(x0, k, K=None, v=None, uact_prev=None, alpha=None, lb=None, ub=None)."""

    def forward(self, x0, k, K=None, v=None, uact_prev=None, alpha=None, lb=None, ub=None):
        return ParamRolloutFn.apply(self.filter, x0, k, K, v, uact_prev, alpha, lb, ub, self.T, self.dt, self.integrator)


class QPSolveFn(torch.autograd.Function):
    """sol, status = QPSolveFn.apply(Hd, c, A, b, lb, ub, be)

    min x'diag(Hd)x + c'x  s.t.  A x >= b (== b for the rows flagged in be), lb <= x <= ub,  one problem per column.
    be: a sequence of nc flags shared by the batch, or None.  nv is 2 or 3 and nc at most 48 (the shapes whose solve and
    adjoint run in registers); anything else raises.  sol [nv,B] is differentiable with respect to all six tensors;
    status int32[B] (1 = solved) is not.  An instance whose status is not 1, or that the backward pass's own solve does
    not decide, gets zero gradients.  Backward is one elementwise select on gsol (the status mask) and one
    asif_hip_qp_vjp_batch launch."""

    @staticmethod
    def forward(ctx, Hd, c, A, b, lb, ub, be):
        if c.dim() != 2 or b.dim() != 2:
            raise ValueError(f"c and b: expected [nv, B] and [nc, B], got {tuple(c.shape)} and {tuple(b.shape)}")
        nv, B = c.shape
        nc = b.shape[0]
        if nv not in (2, 3) or not 1 <= nc <= 48:
            raise ValueError(f"no backward pass for a {nv} x {nc} QP: nv must be 2 or 3 and 1 <= nc <= 48")
        if be is not None and len(be) != nc:
            raise ValueError(f"be: expected {nc} flags, got {len(be)}")
        Hd, c, lb, ub = (_soa(t, nv, B, n) for t, n in ((Hd, "Hd"), (c, "c"), (lb, "lb"), (ub, "ub")))
        A, b = _soa(A, nc * nv, B, "A"), _soa(b, nc, B, "b")
        sol = torch.zeros((nv, B), dtype=torch.float64, device=c.device)
        status = torch.zeros(B, dtype=torch.int32, device=c.device)
        if B > 0:
            capi.qp_solve_batch(Hd, c, A, b, lb, ub, sol, status, be=be, device=c.device.index or 0)
        ctx.be = None if be is None else tuple(int(v) for v in be)
        ctx.save_for_backward(Hd, c, A, b, lb, ub, status)
        ctx.mark_non_differentiable(status)
        return sol, status

    @staticmethod
    def backward(ctx, gsol, _gstatus):
        Hd, c, A, b, lb, ub, status = ctx.saved_tensors
        # Deliberately one elementwise launch in front of the kernel's.  The kernel zeroes the gradients of an instance
        # its OWN solve does not decide; the contract here is about the status the caller saw.  The two agree whenever
        # the forward pass decided in its exact stage, but that pass has other stages (a cost without curvature is
        # solved by its iterations and left undecided here; the reverse, a forward failure next to rc 1, is not ruled
        # out by construction).  Where status != 1, sol carries no value and nothing may flow back: the adjoint is
        # linear in gsol, so a zeroed column yields zero gradients, and a column with status 1 passes through bit for bit.
        gsol = torch.where(status == 1, gsol, torch.zeros_like(gsol)).contiguous()
        grads = [torch.empty_like(t) if need else None
                 for t, need in zip((Hd, c, A, b, lb, ub), ctx.needs_input_grad[:6])]
        if c.shape[1] > 0 and any(g is not None for g in grads):
            gHd, gc, gA, gb, glb, gub = grads
            capi.qp_vjp_batch(Hd, c, A, b, lb, ub, gsol, torch.empty_like(status), gHd=gHd, gc=gc, gA=gA, gb=gb, glb=glb,
                              gub=gub, be=ctx.be, device=c.device.index or 0)
        return (*grads, None)


class QPLayer(torch.nn.Module):
    """A batched small QP in the middle of a model: sol, status = layer(Hd, c, A, b, lb, ub).  Holds the equality
    flags `be` of the rows (None: all inequalities), which belong to the problem's structure, not to its data."""

    def __init__(self, be=None):
        super().__init__()
        self.be = None if be is None else tuple(int(v) for v in be)

    def forward(self, Hd, c, A, b, lb, ub):
        return QPSolveFn.apply(Hd, c, A, b, lb, ub, self.be)
