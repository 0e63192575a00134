"""torch.autograd glue for the native ops that have a gradient: the modules of this package call the plain,
no-grad path for inference and one of these functions when a gradient is being recorded.  Buffer semantics are the native ops'
(outputs and gradients are op-owned and reused by the next call of the same op), as with the reference's own wrappers."""
import torch
from torch.autograd.function import once_differentiable


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def recording(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class UnaryFn(torch.autograd.Function):
    """y = op.forward(x)[0],  dL/dx = op.backward(dL/dy)[0]; `inplace`: the op overwrites x and returns it.
    The in-place ops (apron refresh of SpherePad, SphereTrim) are NOT marked dirty, exactly as the reference's wrappers
    (lic360_operator/SpherePad.py:9-15 returns the op's output, which is its input): autograd then aliases the result to x
    and x's version counter stays put, so a convolution that saved x before the refresh can still run its backward
    (AttentionBlock pads the same x in two branches, ResidualBlockDown pads after the shortcut has saved x).  That is sound
    because the refresh is idempotent on everything an earlier consumer read: it rewrites apron cells with the values a
    previous pad of the same interior already put there, and the trim's zeros are what the reference's graph sees too."""
    @staticmethod
    def forward(ctx, x, op, inplace):
        ctx.op = op
        return op.forward(x)[0]

    @staticmethod
    def backward(ctx, g):
        return ctx.op.backward(_c(g))[0], None, None


class LatScaleFn(torch.autograd.Function):
    """y[n,c,h,w] = x * weight[part(h)]; the band weights get the sum of g * x over their rows"""
    @staticmethod
    def forward(ctx, x, weight, op):
        ctx.op = op
        ctx.save_for_backward(x, weight)
        return op.forward(x, weight)[0]

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = _c(g)
        gx = ctx.op.backward(g, weight)[0]
        npart = weight.numel()
        per_row = (g * x).sum((0, 1, 3))                                    # [h]
        return gx, per_row.view(npart, -1).sum(1).view_as(weight), None


class ImpMapFn(torch.autograd.Function):
    """(x, imp) -> (masked x[, mask], mean level); backward: the op's rule for the importance map, driven by the gap between the
    row-wise mean level and the op's latitude constraint (reference lic360_operator/ImpMap.py:8-57)"""
    @staticmethod
    def forward(ctx, x, imp, level, op, want_mask):
        imp = _c(torch.floor(imp * level) / level)
        out = op.forward(x, imp)
        ctx.op = op
        ctx.save_for_backward(imp, out[1])
        rt = torch.mean(imp)
        if want_mask:
            ctx.mark_non_differentiable(out[2])
            return out[0], out[2], rt
        return out[0], rt

    @staticmethod
    def backward(ctx, g, *unused):
        imp, constrain = ctx.saved_tensors
        gap = _c(torch.mean(imp, dim=3) - constrain)
        gx, gimp = ctx.op.backward(_c(g), imp, gap)
        return gx, gimp, None, None, None


class QuantFn(torch.autograd.Function):
    """(x, weight, count) -> quantised x[, index]; gradients: straight through for x, the op's level-increment gradient for weight,
    and the op's level counts as the "gradient" of count (so that an optimiser step accumulates them; reference QUANT.py:7-28)"""
    @staticmethod
    def forward(ctx, x, weight, count, op, training):
        out = op.forward(x, weight, count, training)
        ctx.op = op
        ctx.save_for_backward(x, out[0])
        return out[0] if len(out) == 1 else (out[0], out[1])

    @staticmethod
    def backward(ctx, *grads):
        x, y = ctx.saved_tensors
        gx, gw, cnt = ctx.op.backward([_c(g) for g in grads], x, y)
        return gx, gw, cnt.clone().detach(), None, None


class ViewportQualityFn(torch.autograd.Function):
    """(a, b) -> (mse, ssim) [n, 14] of lic360.viewport_quality_coef, which keeps coefficient maps only for the sides that need a gradient;
    backward: lic360.viewport_quality_backward from a, b and those maps (no projected view is written in either direction)"""
    @staticmethod
    def forward(ctx, a, b, op, taps):
        import lic360
        ctx.op, ctx.taps, ctx.need = op, taps, tuple(ctx.needs_input_grad[:2])
        mse, ssim, coefs = lic360.viewport_quality_coef(op, a, b, taps, need_a=ctx.need[0], need_b=ctx.need[1])
        ctx.kept = tuple(t is not None for t in coefs)
        ctx.save_for_backward(a, b, *[t for t in coefs if t is not None])
        return mse, ssim

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mse, g_ssim):
        import lic360
        a, b, *maps = ctx.saved_tensors
        maps = iter(maps)
        coefs = tuple(next(maps) if kept else None for kept in ctx.kept)
        ga, gb = lic360.viewport_quality_backward(ctx.op, a, b, ctx.taps, coefs, _c(g_mse), _c(g_ssim), need_a=ctx.need[0], need_b=ctx.need[1])
        return ga, gb, None, None


class GmmRateFn(torch.autograd.Function):
    """(logit, sigma, mean, label, mask) -> (nats [n] float64, symbols [n] int64) of lic360.gmm_rate; saves the inputs only.  backward:
    lic360.gmm_rate_backward recomputes every symbol from them; the label's gradient is asked for only when the label needs one, the mask
    never gets one."""
    @staticmethod
    def forward(ctx, logit, sigma, mean, label, mask):
        import lic360
        nats, symbols = lic360.gmm_rate(logit, sigma, mean, label, mask)
        ctx.need_label = ctx.needs_input_grad[3]
        ctx.save_for_backward(logit, sigma, mean, label, mask)
        ctx.mark_non_differentiable(symbols)
        return nats, symbols

    @staticmethod
    @once_differentiable
    def backward(ctx, g_nats, g_symbols):
        import lic360
        logit, sigma, mean, label, mask = ctx.saved_tensors
        d = lic360.gmm_rate_backward(logit, sigma, mean, label, mask, _c(g_nats.to(torch.float32)), need_label=ctx.need_label)
        return d[0], d[1], d[2], d[3], None


class CeRateFn(torch.autograd.Function):
    """(logit, label) -> (nats [n] float64, symbols [n] int64, invalid [n] int64) of lic360.ce_rate; saves the inputs only.  backward:
    lic360.ce_rate_backward recomputes every symbol from them; the label never gets a gradient."""
    @staticmethod
    def forward(ctx, logit, label):
        import lic360
        nats, symbols, invalid = lic360.ce_rate(logit, label)
        ctx.save_for_backward(logit, label)
        ctx.mark_non_differentiable(symbols, invalid)
        return nats, symbols, invalid

    @staticmethod
    @once_differentiable
    def backward(ctx, g_nats, g_symbols, g_invalid):
        import lic360
        logit, label = ctx.saved_tensors
        return lic360.ce_rate_backward(logit, label, _c(g_nats.to(torch.float32))), None


class MaskConvFn(torch.autograd.Function):
    """(x, weight, bias) -> lic360.cconv_forward: the group-causal 5x5 convolution over an already masked weight, bias added, no activation; saves
    x and the weight.  backward: dx = lic360.cconv_dgrad (the forward kernel on transformed operands; torch's conv2d_input when `dgrad_native` is
    false), only when x needs it; dw = lic360.cconv_wgrad, exact zeros at masked taps; db = the sum of g over n, h, w."""
    @staticmethod
    def forward(ctx, x, weight, bias, ngroup, constrain, dgrad_native):
        import lic360
        ctx.ngroup, ctx.constrain, ctx.dgrad_native = ngroup, constrain, dgrad_native
        ctx.save_for_backward(x, weight)
        return lic360.cconv_forward(x, weight.detach(), bias.detach(), ngroup, constrain)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        import lic360
        x, weight = ctx.saved_tensors
        g = _c(g)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.dgrad_native:
                dx = lic360.cconv_dgrad(g, weight, ctx.ngroup, ctx.constrain)
            else:
                dx = torch.nn.grad.conv2d_input(x.shape, weight, g, padding=2)
        if ctx.needs_input_grad[1]:
            dw = lic360.cconv_wgrad(x, g, ctx.ngroup, ctx.constrain)
        if ctx.needs_input_grad[2]:
            db = g.sum((0, 2, 3))
        return dx, dw, db, None, None, None


class GdnFn(torch.autograd.Function):
    """(x, gamma, beta) -> lic360.gdn_forward on the effective parameters (the bits of the inference forward); saves x, gamma and beta only.
    backward: lic360.gdn_backward recomputes the norm from x and returns what needs_input_grad asks for; the bound / square / pedestal
    reparametrisation in front of gamma and beta stays torch work and carries these gradients on to the raw parameters."""
    @staticmethod
    def forward(ctx, x, gamma, beta, inverse):
        import lic360
        ctx.inverse = bool(inverse)
        ctx.save_for_backward(x, gamma, beta)
        return lic360.gdn_forward(x, gamma.detach(), beta.detach(), ctx.inverse)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        import lic360
        x, gamma, beta = ctx.saved_tensors
        need_params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gx, gg, gb = lic360.gdn_backward(x, _c(g), gamma, beta, ctx.inverse, need_x=ctx.needs_input_grad[0], need_params=need_params)
        return gx, gg if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None
