"""The explicit safety filter (class ASIF) as a differentiable torch layer.

Forward: asif_hip_filter_batch / asif_hip_filter_batch_lie.  Backward: one asif_hip_filter_vjp_batch launch
(asif_amd/csrc/k_explicit_vjp.hip).  Both run on torch's current stream; nothing here computes on the CPU and
nothing falls back to torch operators.

Tensors are FP64 CUDA tensors, structure-of-arrays: x [nx,B], udes [nu,B], lfh [nc,B], lgh [nc*nu,B].
"""
import torch

from . import capi


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
