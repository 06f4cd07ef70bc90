"""torch.autograd bindings of the hand-written HIP kernels used by the training step."""
import torch

from .. import _native


class _InstNormLReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope, eps):
        x = x.contiguous()
        B, C = x.shape[0], x.shape[1]
        hw = x.numel() // (B * C)
        dtype = {torch.float32: 0, torch.bfloat16: 1}[x.dtype]
        y = torch.empty_like(x)
        mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        w = weight.float().contiguous() if weight is not None else None
        b = bias.float().contiguous() if bias is not None else None
        _native.launch("octa_instnorm_lrelu_fwd", x.device, x, y, w, b, mean, rstd, B, C, hw, dtype, float(slope), float(eps))
        ctx.save_for_backward(x, w, b, mean, rstd)
        ctx.slope, ctx.has_w, ctx.has_b = float(slope), weight is not None, bias is not None
        ctx.w_dtype = weight.dtype if weight is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        B, C = x.shape[0], x.shape[1]
        hw = x.numel() // (B * C)
        dtype = {torch.float32: 0, torch.bfloat16: 1}[x.dtype]
        dx = torch.empty_like(x)
        dw = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_w else None
        db = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_b else None
        _native.launch("octa_instnorm_lrelu_bwd", x.device, x, dy, w, b, mean, rstd, dx, dw, db, B, C, hw, dtype, ctx.slope)
        return dx, (dw.to(ctx.w_dtype) if dw is not None else None), (db.to(ctx.w_dtype) if db is not None else None), None, None


def instance_norm_leaky_relu(x, weight, bias, negative_slope=0.01, eps=1e-5):
    """InstanceNorm2d(affine) followed by LeakyReLU in one HIP pass pair (CUDA tensors, float32 or bfloat16)."""
    return _InstNormLReLU.apply(x, weight, bias, negative_slope, eps)
