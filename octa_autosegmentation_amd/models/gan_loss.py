"""The elementwise tail of the CycleGAN step (models/cycle_gan.py) on the kernels of csrc/gan_loss.hip: weighted L1 terms, LSGAN
terms, background mixing and the image pool's exchange. As torch operations the tail is a chain of short dependent launches on small
tensors (sub, abs, mean, scale and their backward per L1 term, the same per LSGAN term, product + maximum, one clone per pooled
image); here every group of terms is one call each way.

Every kernel has a host restatement in plain torch next to it (`*_host`): the same arithmetic, rounding by rounding. CPU tensors run
the restatement (there is no CPU build of the kernels), the GPU tests use it as the oracle. `USE_FUSED_GAN_LOSS = False` runs the
ordinary torch composition (autograd's own backward) on the GPU instead of the kernels -- the yardstick of tools/time_cyclegan.py and
of tests/test_cycle_gan_gpu.py.

Gradients: `l1_pairs` and `lsgan` return (total, values); only the TOTAL carries a gradient, the values are for reporting."""
import ctypes

import torch

USE_FUSED_GAN_LOSS = True

L1_MAX_TERMS, LSGAN_MAX_TERMS, POOL_MAX_BATCH = 4, 2, 32
_CODES = {torch.float32: 0, torch.bfloat16: 1}


def _code(t):
    if t.dtype not in _CODES:
        raise TypeError(f"csrc/gan_loss.hip takes float32 and bfloat16 tensors, not {t.dtype}")
    return _CODES[t.dtype]


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _on_kernels(t):
    return t.is_cuda and USE_FUSED_GAN_LOSS


# ---- weighted L1 terms ---------------------------------------------------------------------------------------------------------------

def l1_pairs_sums_host(preds, targets):
    """double[K]: sum |pred_k - target_k|, differences and sums in float64."""
    return torch.stack([(p.double() - t.double()).abs().sum() for p, t in zip(preds, targets)])


def l1_pairs_finish_host(sums, ns, ws):
    """float32[K + 1]: w_k sums_k / n_k and their total (added in float64, rounded once)."""
    v = sums.double() * torch.tensor(ws, dtype=torch.float64, device=sums.device) / torch.tensor(ns, dtype=torch.float64, device=sums.device)
    return torch.cat((v, v.sum().reshape(1))).float()


def l1_pairs_bwd_host(g, preds, targets, ws):
    """d pred_k = (g * float32(w_k / n_k)) * sign(pred_k - target_k) in pred's dtype; sign(0) = 0 like torch's l1_loss."""
    out = []
    for p, t, w in zip(preds, targets, ws):
        c = g.reshape(()).float() * torch.tensor(w / p.numel(), dtype=torch.float32, device=p.device)
        s = (p.float() > t.float()).float() - (p.float() < t.float()).float()
        out.append((c * s).to(p.dtype))
    return out


def l1_pairs_sums_device(preds, targets, sums=None):
    from .. import _native
    dev, K = preds[0].device, len(preds)
    sums = torch.empty(K, dtype=torch.float64, device=dev) if sums is None else sums
    _native.launch("octa_l1_pairs_fwd", dev, K, _ptrs(preds), _ptrs(targets), _arr(ctypes.c_int64, [p.numel() for p in preds]), _code(preds[0]),
                   _code(targets[0]), sums)
    return sums


def l1_pairs_finish_device(sums, ns, ws, out=None):
    from .. import _native
    out = torch.empty(len(ns) + 1, dtype=torch.float32, device=sums.device) if out is None else out
    _native.launch("octa_l1_pairs_finish", sums.device, len(ns), sums, _arr(ctypes.c_int64, ns), _arr(ctypes.c_double, ws), out)
    return out


def l1_pairs_bwd_device(g, preds, targets, ws, dpreds=None):
    from .. import _native
    dev, K = preds[0].device, len(preds)
    dpreds = [torch.empty_like(p) for p in preds] if dpreds is None else dpreds
    gg = g.reshape(1).float().contiguous()
    _native.launch("octa_l1_pairs_bwd", dev, K, _ptrs(preds), _ptrs(targets), _arr(ctypes.c_int64, [p.numel() for p in preds]), _arr(ctypes.c_double, ws),
                   _code(preds[0]), _code(targets[0]), gg, _ptrs(dpreds))
    return dpreds


def _check_terms(tensors, others, limit, what):
    if not 1 <= len(tensors) <= limit:
        raise ValueError(f"{what}: 1 to {limit} terms per call, got {len(tensors)}")
    for a, b in zip(tensors, others):
        if b is not None and a.shape != b.shape:
            raise ValueError(f"{what}: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
        if a.numel() == 0:
            raise ValueError(f"{what}: empty tensor")


class _L1Pairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ws, *tensors):
        preds, targets = [t.contiguous() for t in tensors[0::2]], [t.contiguous() for t in tensors[1::2]]
        ns = [p.numel() for p in preds]
        if _on_kernels(preds[0]):
            out = l1_pairs_finish_device(l1_pairs_sums_device(preds, targets), ns, ws)
        else:
            out = l1_pairs_finish_host(l1_pairs_sums_host(preds, targets), ns, ws)
        ctx.ws, ctx.on_kernels = ws, _on_kernels(preds[0])
        ctx.save_for_backward(*preds, *targets)
        total, values = out[len(ns)], out[:len(ns)]
        ctx.mark_non_differentiable(values)
        return total, values

    @staticmethod
    def backward(ctx, g, _):
        K = len(ctx.ws)
        preds, targets = ctx.saved_tensors[:K], ctx.saved_tensors[K:]
        d = (l1_pairs_bwd_device if ctx.on_kernels else l1_pairs_bwd_host)(g, list(preds), list(targets), ctx.ws)
        grads = [None]
        for k in range(K):
            grads += [d[k] if ctx.needs_input_grad[1 + 2 * k] else None, None]
        return tuple(grads)


def l1_pairs(terms):
    """terms: up to four (pred, target, weight). Returns (sum_k weight_k * mean |pred_k - target_k|, the K terms as a float32 vector)."""
    preds, targets, ws = [t[0] for t in terms], [t[1] for t in terms], tuple(float(t[2]) for t in terms)
    _check_terms(preds, targets, L1_MAX_TERMS, "l1_pairs")
    if preds[0].is_cuda and not USE_FUSED_GAN_LOSS:
        vals = [w * torch.nn.functional.l1_loss(p.float(), t.float()) for p, t, w in zip(preds, targets, ws)]
        return sum(vals), torch.stack([v.detach() for v in vals])
    if len({p.dtype for p in preds}) > 1:              # one dtype per launch: mixed lists go up to float32 (autograd brings the gradient back)
        preds = [p.float() for p in preds]
    if len({t.dtype for t in targets}) > 1:
        targets = [t.float() for t in targets]
    flat = [x for pair in zip(preds, targets) for x in pair]
    return _L1Pairs.apply(ws, *flat)


# ---- LSGAN terms ---------------------------------------------------------------------------------------------------------------------

def lsgan_host(ps, targets, scales):
    """(double[T] sums of (p_k - target_k)^2 in float64, float32[T + 1] scale_k sums_k / n_k and their total)."""
    sums = torch.stack([((p.double() - float(t)) ** 2).sum() for p, t in zip(ps, targets)])
    v = sums * torch.tensor(scales, dtype=torch.float64, device=sums.device) / torch.tensor([p.numel() for p in ps], dtype=torch.float64, device=sums.device)
    return sums, torch.cat((v, v.sum().reshape(1))).float()


def lsgan_bwd_host(g, ps, targets, scales):
    """d p_k = (g * float32(2 scale_k / n_k)) * (p_k - target_k) in float32 arithmetic, rounded to p's dtype."""
    out = []
    for p, t, s in zip(ps, targets, scales):
        c = g.reshape(()).float() * torch.tensor(2.0 * s / p.numel(), dtype=torch.float32, device=p.device)
        out.append((c * (p.float() - float(t))).to(p.dtype))
    return out


def lsgan_device(ps, targets, scales, sums=None, loss=None):
    from .. import _native
    dev, T = ps[0].device, len(ps)
    sums = torch.empty(T, dtype=torch.float64, device=dev) if sums is None else sums
    loss = torch.empty(T + 1, dtype=torch.float32, device=dev) if loss is None else loss
    _native.launch("octa_lsgan_fwd", dev, T, _ptrs(ps), _arr(ctypes.c_int64, [p.numel() for p in ps]), _arr(ctypes.c_float, targets),
                   _arr(ctypes.c_double, scales), _code(ps[0]), sums, loss)
    return sums, loss


def lsgan_bwd_device(g, ps, targets, scales, dps=None):
    from .. import _native
    dev, T = ps[0].device, len(ps)
    dps = [torch.empty_like(p) for p in ps] if dps is None else dps
    gg = g.reshape(1).float().contiguous()
    _native.launch("octa_lsgan_bwd", dev, T, _ptrs(ps), _arr(ctypes.c_int64, [p.numel() for p in ps]), _arr(ctypes.c_float, targets),
                   _arr(ctypes.c_double, scales), _code(ps[0]), gg, _ptrs(dps))
    return dps


class _Lsgan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, scales, *ps):
        ps = [p.contiguous() for p in ps]
        ctx.on_kernels = _on_kernels(ps[0])
        _, out = (lsgan_device if ctx.on_kernels else lsgan_host)(ps, targets, scales)
        ctx.targets, ctx.scales = targets, scales
        ctx.save_for_backward(*ps)
        total, values = out[len(ps)], out[:len(ps)]
        ctx.mark_non_differentiable(values)
        return total, values

    @staticmethod
    def backward(ctx, g, _):
        d = (lsgan_bwd_device if ctx.on_kernels else lsgan_bwd_host)(g, list(ctx.saved_tensors), ctx.targets, ctx.scales)
        return (None, None) + tuple(d[k] if ctx.needs_input_grad[2 + k] else None for k in range(len(d)))


def lsgan(terms):
    """terms: up to two (prediction, target_is_real, scale). Returns (sum_k scale_k * mean (p_k - target_k)^2, the T terms as a float32 vector)."""
    ps, targets, scales = [t[0] for t in terms], tuple(1.0 if t[1] else 0.0 for t in terms), tuple(float(t[2]) for t in terms)
    _check_terms(ps, [None] * len(ps), LSGAN_MAX_TERMS, "lsgan")
    if ps[0].is_cuda and not USE_FUSED_GAN_LOSS:
        vals = [s * torch.nn.functional.mse_loss(p.float(), torch.full_like(p, t, dtype=torch.float32)) for p, t, s in zip(ps, targets, scales)]
        return sum(vals), torch.stack([v.detach() for v in vals])
    if len({p.dtype for p in ps}) > 1:
        ps = [p.float() for p in ps]
    return _Lsgan.apply(targets, scales, *ps)


# ---- background mixing ---------------------------------------------------------------------------------------------------------------

def mix_max_host(x, bg, u):
    """max(x, bg * u): the product rounded in bg's dtype, the result in torch's promoted dtype."""
    return torch.maximum(x, bg * u)


def mix_max_bwd_host(x, bg, u, dout):
    """torch's rule for maximum: the whole gradient where x > m, half of it at ties, none where x < m."""
    m = bg * u
    xf, mf, d = x.float(), m.float(), dout.float()
    return torch.where(xf > mf, d, torch.where(xf == mf, 0.5 * d, torch.zeros_like(d))).to(x.dtype)


def _mix_out_dtype(x, bg):
    return torch.bfloat16 if x.dtype == torch.bfloat16 and bg.dtype == torch.bfloat16 else torch.float32


def mix_max_device(x, bg, u, out=None):
    from .. import _native
    out = torch.empty(x.shape, dtype=_mix_out_dtype(x, bg), device=x.device) if out is None else out
    _native.launch("octa_mix_max_fwd", x.device, x, _code(x), bg, u, _code(bg), x.numel(), out)
    return out


def mix_max_bwd_device(x, bg, u, dout, dx=None):
    from .. import _native
    dx = torch.empty_like(x) if dx is None else dx
    _native.launch("octa_mix_max_bwd", x.device, x, _code(x), bg, u, _code(bg), x.numel(), dout, dx)
    return dx


class _MixMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bg, u):
        x, bg, u = x.contiguous(), bg.contiguous(), u.contiguous()
        ctx.on_kernels = _on_kernels(x)
        ctx.save_for_backward(x, bg, u)
        return (mix_max_device if ctx.on_kernels else mix_max_host)(x, bg, u)

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x, bg, u = ctx.saved_tensors
        dout = dout.to(_mix_out_dtype(x, bg)).contiguous()
        return (mix_max_bwd_device if ctx.on_kernels else mix_max_bwd_host)(x, bg, u, dout), None, None


def mix_max(x, bg, u):
    """max(x, bg * u) for tensors of one shape; bg and u carry no gradient."""
    if not (x.shape == bg.shape == u.shape) or x.numel() == 0:
        raise ValueError(f"mix_max: shapes {tuple(x.shape)}, {tuple(bg.shape)}, {tuple(u.shape)}")
    if x.is_cuda and not USE_FUSED_GAN_LOSS:
        return torch.maximum(x, bg * u)
    if bg.dtype != u.dtype:                     # torch's promotion of bg * u
        dt = torch.promote_types(bg.dtype, u.dtype)
        bg, u = bg.to(dt), u.to(dt)
    return _MixMax.apply(x, bg.detach(), u.detach())


# ---- image pool ----------------------------------------------------------------------------------------------------------------------

def pool_exchange_host(pool, images, src, wslot, winput):
    """Apply one resolved query: the returned images are gathered BEFORE the slots are overwritten."""
    out = torch.stack([images[s] if s >= 0 else pool[-1 - s] for s in src])
    for s, k in zip(wslot, winput):
        pool[s] = images[k]
    return out


def pool_exchange_device(pool, images, src, wslot, winput, out=None):
    from .. import _native
    out = torch.empty_like(images) if out is None else out
    _native.launch("octa_pool_exchange", images.device, pool, pool.shape[0], images, images.shape[0], out, images[0].numel(), _code(images),
                   _arr(ctypes.c_int, src), len(wslot), _arr(ctypes.c_int, wslot), _arr(ctypes.c_int, winput))
    return out
