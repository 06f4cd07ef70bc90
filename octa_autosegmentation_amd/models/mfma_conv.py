"""Host side of the hand-written MFMA convolution (csrc/conv.hip): NHWC bf16 tensors in, NHWC bf16 out.

Layouts: activations [N, H, W, C] contiguous bfloat16; weights "tap-major" [9, Cout, Cin] bfloat16 (tap = 3*r+s).
`fwd_layout` / `dgrad_layout` convert a torch conv weight [Cout, Cin, K, K] (models/networks.py, MONAI DynUNet naming) into the
forward layout and into the layout whose forward pass IS the data gradient (pure torch, any device); `pack_weight` /
`pack_weight_dgrad` / `pack_convt2x2` serve the same bits from the network's WeightPackPlan when the parameter is registered in one.
"""
import ctypes
import os

import torch

from .. import _native
from . import weight_cache


def _pad32(c):
    return (c + 31) // 32 * 32


def _zero_pad(t, dim, size):
    """t with axis `dim` zero-padded to `size` entries (t itself when it has them already)."""
    if t.shape[dim] == size:
        return t
    shape = list(t.shape)
    shape[dim] = size
    out = t.new_zeros(shape)
    out.narrow(dim, 0, t.shape[dim]).copy_(t)
    return out


def _bf16c(t):
    """Contiguous bfloat16 (the form every backward kernel reads its incoming gradient in)."""
    t = t.contiguous()
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


def _conv3x3_fwd(x, wt, y, x2=None, y2=None, stride=1, in_dilation=1, tap_mask=0x1ff, scatter=(1, 0, 0), norm=(None, None, None, None), slope=0.0,
                 stat_partials=None, stat_slots=None, residual=None, what="octa_conv3x3_nhwc_fwd"):
    """One launch of octa_conv3x3_nhwc_fwd: x (| x2 on the channel axis) [N,H,W,C] -> y (| y2), all bf16; wt packed [9][Cout][Cin]. scatter =
    (out_scale, out_off_y, out_off_x); norm = (scale1, shift1, scale2, shift2) of the normalise-on-load inputs; stat_partials float32
    [N][tiles][Cout][2] / stat_slots double [nslot][N][Cout][2] receive the InstanceNorm sums of the result; residual is added in the epilogue."""
    n, h, w, c1 = x.shape
    ad = _native.addr
    a = _native.Conv3x3Args(
        struct_size=ctypes.sizeof(_native.Conv3x3Args), N=n, H=h, W=w, Cin=c1 + (x2.shape[3] if x2 is not None else 0),
        Cout=y.shape[3] + (y2.shape[3] if y2 is not None else 0), stride=int(stride), in_dilation=int(in_dilation), tap_mask=int(tap_mask),
        out_scale=int(scatter[0]), out_off_y=int(scatter[1]), out_off_x=int(scatter[2]), C1=c1, CY1=y.shape[3],
        nslot=stat_slots.shape[0] if stat_slots is not None else 0, slope=float(slope), d_x=ad(x), d_x2=ad(x2), d_w=ad(wt), d_y=ad(y),
        d_y2=ad(y2), d_scale1=ad(norm[0]), d_shift1=ad(norm[1]), d_scale2=ad(norm[2]), d_shift2=ad(norm[3]),
        d_stat_partials=ad(stat_partials), d_stat_slots=ad(stat_slots), d_residual=ad(residual))
    _native.launch("octa_conv3x3_nhwc_fwd", x.device, ctypes.byref(a), what=what)


def _conv3x3_wgrad(x1, dy, x2=None, into=None, accumulate=False, stride=1, tap_mask=0x1ff, norm=(None, None, None, None), slope=0.0):
    """One launch of octa_conv3x3_nhwc_wgrad for the layer with input x1 (| x2 on the channel axis) and output gradient dy. into = None: returns dW
    [Cout, Cin, 3, 3] float32 (a view of the kernel's tap-major result; taps cleared in tap_mask are zero); into = a float32 gradient buffer in the
    parameter layout [Cout][Cin][3][3]: the result is added to it (accumulate) or written over it."""
    n, h, w, c1 = x1.shape
    cin, cout = c1 + (x2.shape[3] if x2 is not None else 0), dy.shape[3]
    dw = into if into is not None else torch.empty((9, cout, cin), dtype=torch.float32, device=x1.device)
    mode = _native.WGRAD_TAP_MAJOR if into is None else (_native.WGRAD_PARAM_ADD if accumulate else _native.WGRAD_PARAM_SET)
    ad = _native.addr
    a = _native.Conv3x3WgradArgs(
        struct_size=ctypes.sizeof(_native.Conv3x3WgradArgs), N=n, H=h, W=w, Cin=cin, Cout=cout, stride=int(stride), tap_mask=int(tap_mask), C1=c1,
        out_mode=mode, slope=float(slope), d_x=ad(x1), d_x2=ad(x2), d_dy=ad(dy), d_dw=ad(dw), d_scale1=ad(norm[0]),
        d_shift1=ad(norm[1]), d_scale2=ad(norm[2]), d_shift2=ad(norm[3]))
    _native.launch("octa_conv3x3_nhwc_wgrad", x1.device, ctypes.byref(a))
    return None if into is not None else dw.view(3, 3, cout, cin).permute(2, 3, 0, 1)


# ---- weight gradients on a side stream ---------------------------------------------------------------------------------
# Weight gradients straight into `weight.grad` (round 5). A layer's weight gradient is a leaf of the backward graph: nothing reads it
# before the optimiser step. Inside `direct_weight_grads()` (the trainers wrap `loss.backward()` in it, models/base_model_abc.py
# backward_scope) the 3x3 weight-gradient launches write their result into the parameter's `.grad` in the parameter's own layout
# (csrc/conv.hip octa_conv3x3_nhwc_wgrad, out_mode OCTA_WGRAD_PARAM_ADD / _SET) -- ADDED to an existing gradient (a view of the data-parallel gradient arena, a second use
# of the weight), written over a fresh buffer otherwise -- and the Function reports None to autograd: no [9][Cout][Cin] temporary, no
# fill, no layout copy and no accumulation launch per layer (21 copies + 15 fills per U-Net step, ~3 per convolution of the GAN's
# generator). Outside the context (tests, torch.autograd.grad, user code calling
# .backward() directly) and for parameters without a matching float32 `.grad` the gradient is returned to autograd as before.
# (Measured and removed in round 5: the same scope running the weight-gradient launches on a SIDE STREAM beside the data-gradient / norm
# chain -- U-Net step 19.3 against 19.0 ms at B = 4, 38.7 against 35.5 at B = 8, profiles/r05_stream_overlap_ab.log: every kernel of the
# step fills the GPU on its own, co-resident workgroups only evict each other's lines.)
USE_DIRECT_WGRAD = True         # module switch (tests / tools may clear it): every gradient then returns through autograd
# set by direct_weight_grads(); read by the autograd ENGINE's thread (not the caller's: a thread-local would never be seen there), hence
# process-wide -- and hence one backward scope at a time: a second thread entering while one is open is refused (its backward would get
# None for its weight gradients and find them written into .grad), torch.autograd.grad / .backward() outside a scope are unaffected
_WG_ACTIVE = {"on": False, "owner": None}
DIRECT_WGRAD_COUNTS = [0, 0]    # weight gradients accumulated in place / returned to autograd


class direct_weight_grads:
    """with direct_weight_grads(device): loss.backward()"""

    def __init__(self, device):
        self.on = USE_DIRECT_WGRAD and torch.device(device).type == "cuda"

    def __enter__(self):
        import threading
        me = threading.get_ident()
        self.prev = (_WG_ACTIVE["on"], _WG_ACTIVE["owner"])
        if self.on:
            if _WG_ACTIVE["on"] and _WG_ACTIVE["owner"] not in (None, me):
                raise RuntimeError("direct_weight_grads(): another thread is inside a backward scope; the in-place weight gradients need one backward at a time "
                                   "(mfma_conv.USE_DIRECT_WGRAD = False returns every gradient through autograd)")
            _WG_ACTIVE["on"], _WG_ACTIVE["owner"] = True, me
        return self

    def __exit__(self, *exc):
        _WG_ACTIVE["on"], _WG_ACTIVE["owner"] = self.prev
        return False


def _wgrad_to(weight, fn, into=None):
    """dW for `weight`: inside direct_weight_grads() `into(grad, accumulate)` writes the gradient into the parameter's float32 `.grad` in
    place -- added to an existing one, written over a fresh buffer when there is none -- and None goes back to autograd; otherwise
    fn()'s tensor does."""
    if into is not None and _WG_ACTIVE["on"] and weight.is_leaf and weight.is_cuda and weight.dtype == torch.float32:
        g = weight.grad
        if g is None:
            g = torch.empty_like(weight, memory_format=torch.contiguous_format)
            into(g, 0)
            weight.grad = g
            DIRECT_WGRAD_COUNTS[0] += 1
            return None
        if g.dtype == torch.float32 and g.is_contiguous() and g.shape == weight.shape:
            into(g, 1)
            DIRECT_WGRAD_COUNTS[0] += 1
            return None
    DIRECT_WGRAD_COUNTS[1] += 1
    return fn()


def _wgrad_acc(x1, x2, dy, grad, accumulate, stride=1, tap_mask=0x1ff):
    """grad [Cout][Cin][3][3] float32 (+)= weight gradient of the 3x3 layer with input x1 (| x2 on the channel axis) and output gradient dy."""
    _conv3x3_wgrad(x1, dy, x2, into=grad, accumulate=accumulate, stride=stride, tap_mask=tap_mask)


class WeightPackPlan:
    """All KxK convolution weights of a network packed into both kernel layouts by ONE launch per optimiser step
    (csrc/conv.hip octa_pack_conv_weights) instead of ~7 small torch kernels per layer and step. The plan is
    refreshed when any parameter's version counter (or storage) changed or the invalidation epoch moved; `pack_weight*` below
    look parameters up here and fall back to the torch formulation for tensors that are not registered. Optimisers,
    `load_state_dict` and every in-place op on the parameter move the counter; writes through `parameter.data` do NOT -- call
    `weight_cache.invalidate()` after those (`networks.init_weights` does). One buffer and one launch for all parameters: the plan
    keeps the staleness rule of weight_cache.cached() for the whole list instead of a cache slot per parameter."""

    def __init__(self, convs, convts=()):
        """convs: float32 parameters [Cout,Cin,K,K]; convts: ConvTranspose2d(2, 2) parameters [Cin,Cout,2,2]."""
        self.params = [(w, 0) for w in convs] + [(w, 1) for w in convts]
        assert all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() for w, _ in self.params)
        self.device = self.params[0][0].device
        off, self.geom = 0, []
        for w, kind in self.params:
            a, b = w.shape[0], w.shape[1]
            kk = 9 if kind == 1 else w.shape[2] * w.shape[3]
            bp = _pad32(b)
            n = kk * a * bp
            self.geom.append((off, off + n, a, b, bp, kk, kind))
            off += 2 * n
        self.buf = torch.empty(off, dtype=torch.bfloat16, device=self.device)
        self.fwd = [self.buf[g[0]:g[0] + g[5] * g[2] * g[4]].view(g[5], g[2], g[4]) for g in self.geom]      # [KK][A][BP]
        self.dg = [self.buf[g[1]:g[1] + g[5] * g[2] * g[4]].view(g[5], g[4], g[2]) for g in self.geom]       # [KK][BP][A]
        self.table, self.ptrs, self.versions = None, None, None
        for i, (w, _) in enumerate(self.params):
            w._octa_pack = (self, i)          # found again by pack_weight*(w); lives as long as the parameter

    def ensure(self):
        ptrs = [w.data_ptr() for w, _ in self.params]
        versions = (weight_cache.epoch(), [w._version for w, _ in self.params])
        if ptrs != self.ptrs:
            # storage moved (.to(), .bfloat16(), memory_format change ...): the packing kernel reads contiguous fp32 [A][B][K][K]
            for w, _ in self.params:
                if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
                    raise RuntimeError("MFMA weight packing needs contiguous float32 master weights on the GPU; got "
                                       f"{w.dtype}, contiguous={w.is_contiguous()}, device={w.device} (convert activations, not parameters)")
            rows = [[p, g[0], g[1], g[2], g[3], g[4], g[5], g[6]] for p, g in zip(ptrs, self.geom)]
            self.table = torch.tensor(rows, dtype=torch.int64).to(self.device)
            self.ptrs, self.versions = ptrs, None
        if versions != self.versions:
            _native.launch("octa_pack_conv_weights", self.device, self.table, len(self.params), self.buf)
            self.versions = versions


def plan_for_module(module):
    """One WeightPackPlan over every MFMA-shaped convolution weight of `module` (3x3 / 4x4 Conv2d, 2x2 ConvTranspose2d),
    built on first use and cached on the module; None when nothing qualifies (CPU, non-float32 master weights)."""
    plan = getattr(module, "_octa_pack_plan", None)
    if plan is not None:
        return plan
    ok = lambda w: w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    convs = [m.weight for m in module.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size in ((3, 3), (4, 4)) and m.groups == 1
             and ok(m.weight)]
    convts = [m.weight for m in module.modules() if isinstance(m, torch.nn.ConvTranspose2d) and m.kernel_size == (2, 2) and m.stride == (2, 2)
              and m.groups == 1 and ok(m.weight)]
    if not convs and not convts:
        return None
    plan = WeightPackPlan(convs, convts)
    object.__setattr__(module, "_octa_pack_plan", plan)
    return plan


def _planned(w, kind):
    ent = getattr(w, "_octa_pack", None)
    if ent is None or ent[0].params[ent[1]][0] is not w or ent[0].params[ent[1]][1] != kind:
        return None, None
    ent[0].ensure()
    return ent


def slice_major(wt):
    """Tap-major packed weights [KK][Cout][CinP] -> the storage order the kernels read, [CinP/16][KK][Cout][16] (csrc/conv.hip wt_off():
    the 16 input channels of one MFMA K-step are contiguous for all taps and output channels, so a workgroup's weight slice is whole
    cache lines). The nominal shape stays [KK][Cout][CinP] -- the tensor is only ever handed to the kernels."""
    kk, co, cp = wt.shape
    assert cp % 16 == 0, "packed weights: input channels must be a multiple of 16"
    return wt.reshape(kk, co, cp // 16, 16).permute(2, 0, 1, 3).contiguous().view(kk, co, cp)


def tap_major(wt):
    """Inverse of slice_major(): the nominal [KK][Cout][CinP] view of packed weights (tests, debugging)."""
    kk, co, cp = wt.shape
    return wt.reshape(cp // 16, kk, co, 16).permute(1, 2, 0, 3).reshape(kk, co, cp)


# ---- the two kernel layouts of a weight, pure torch (any device; no cache, no plan) ---------------------------------------

def fwd_layout(w, cin_pad=None):
    """[Cout, Cin, K, K] -> [K*K, Cout, CinP] bf16 (CinP = cin_pad or Cin; padded columns zero), stored slice-major (slice_major())."""
    w = _zero_pad(w, 1, w.shape[1] if cin_pad is None else cin_pad)
    return slice_major(w.permute(2, 3, 0, 1).reshape(w.shape[2] * w.shape[3], w.shape[0], w.shape[1]).to(torch.bfloat16))


def dgrad_layout(w, cin_pad=None):
    """[Cout, Cin, K, K] -> [K*K, CinP, Cout] bf16 with the taps flipped: conv(dy, this) = dL/dx."""
    w = _zero_pad(w, 1, w.shape[1] if cin_pad is None else cin_pad)
    return slice_major(w.flip(2, 3).permute(2, 3, 1, 0).reshape(w.shape[2] * w.shape[3], w.shape[1], w.shape[0]).to(torch.bfloat16))


def convt2x2_layouts(w):
    """ConvTranspose2d(2, 2) weight [Cin, Cout, 2, 2] as the 3x3 kernel wc[a][b][r][s] = w[a][b][r-1][s-1] (zero at r = 0 or
    s = 0), in both layouts: (fwd_layout(wc) [9, Cin, Cout], dgrad_layout(wc) [9, Cout, Cin])."""
    wc = w.new_zeros((w.shape[0], w.shape[1], 3, 3))
    wc[:, :, 1:, 1:] = w
    return fwd_layout(wc), dgrad_layout(wc)


# ---- the same layouts of a parameter: from its WeightPackPlan when it is registered in one, else computed ------------------

def pack_weight(w, cin_pad=None):
    """fwd_layout(w, cin_pad) of a parameter."""
    plan, i = _planned(w, 0)
    if plan is not None and plan.geom[i][4] == (w.shape[1] if cin_pad is None else cin_pad):
        return plan.fwd[i]
    return fwd_layout(w, cin_pad)


def pack_weight_dgrad(w, cin_pad=None):
    """dgrad_layout(w, cin_pad) of a parameter."""
    plan, i = _planned(w, 0)
    if plan is not None and plan.geom[i][4] == (w.shape[1] if cin_pad is None else cin_pad):
        return plan.dg[i]
    return dgrad_layout(w, cin_pad)


def pack_convt2x2(w):
    """convt2x2_layouts(w) of a parameter."""
    plan, i = _planned(w, 1)
    if plan is not None and plan.geom[i][4] == w.shape[1]:
        return plan.fwd[i], plan.dg[i]
    return convt2x2_layouts(w)


def conv3x3_nhwc(x, wt, stride=1, in_dilation=1, tap_mask=0x1ff, residual=None):
    """x [N,H,W,Cin] bf16, wt [9,Cout,Cin] bf16 -> [N,Ho,Wo,Cout] bf16 (padding 1). tap_mask bit 3r+s = evaluate tap
    (r, s) of wt (as packed); cleared taps must have zero weights. residual (shape of the result, bf16) is added in the
    kernel's epilogue."""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4
    assert wt.dtype == torch.bfloat16 and wt.is_contiguous() and wt.shape[0] == 9 and wt.shape[2] == x.shape[3]
    n, h, w, _ = x.shape
    cout = wt.shape[1]
    ho = (h * in_dilation - 1) // stride + 1
    wo = (w * in_dilation - 1) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == torch.bfloat16 and residual.is_contiguous()
    _conv3x3_fwd(x, wt, y, stride=stride, in_dilation=in_dilation, tap_mask=tap_mask, residual=residual)
    return y


# The parity-fused kernel for the two layers that double the image (round 5, csrc/conv.hip conv3x3_s2t_kernel): the data gradient of a
# stride-2 layer and the 2x2 transposed convolution. Rounds 1-4 ran them as conv3x3_nhwc(..., in_dilation=2), the stride-1 kernel on a
# virtually zero-inserted input (4 x the multiply-adds; _ConvLazy.backward still does). Four scattered launches, one per output parity
# (scatter=(2, a, b); drivers in tests/test_conv_gpu.py), measured no faster than that form on MI355X, B = 4, 1216^2 U-Net step:
# 32.6 vs 32.1 ms (register-staged kernels); stride-2 data gradient 22.0 vs 21.8 ms, transposed convolution 22.15 vs 21.8 ms (DMA-staged).
def conv3x3_s2t_nhwc(x, wt, tap_mask=0x1ff, residual=None):
    """x [N,H,W,Cin] bf16 (the small image), wt [9,Cout,Cin] bf16 as conv3x3_nhwc(..., in_dilation=2) takes it -> [N,2H,2W,Cout] bf16."""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and wt.dtype == torch.bfloat16 and wt.is_contiguous() and wt.shape[2] == x.shape[3]
    n, h, w, cin = x.shape
    cout = wt.shape[1]
    y = torch.empty((n, 2 * h, 2 * w, cout), dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == torch.bfloat16 and residual.is_contiguous()
    _native.launch("octa_conv3x3_s2t_nhwc", x.device, x, wt, y, n, h, w, cin, cout, int(tap_mask), residual)
    return y


def conv3x3_nhwc_wgrad(x, dy, tap_mask=0x1ff):
    """x [N,H,W,Cin] bf16, dy [N,H,W,Cout] bf16 (stride-1 layer) -> dW as a torch conv weight gradient
    [Cout, Cin, 3, 3] float32 (taps cleared in tap_mask come back as zero)."""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and dy.dtype == torch.bfloat16 and dy.is_contiguous()
    assert dy.shape[:3] == x.shape[:3]
    return _conv3x3_wgrad(x, dy, tap_mask=tap_mask)


STAT_SLOTS = 16      # slots the tiles of an image spread their statistics atomics over
_STAT_RINGS = {}
_STAT_LOCK = __import__("threading").Lock()                  # two threads running forwards on one stream must not be handed overlapping slices


def _stat_slots(device, n, cout):
    """Zeroed double[STAT_SLOTS][n][cout][2] from a per-(device, stream) ring: ONE fill per lap instead of one per layer. A slice is
    consumed by the two launches enqueued right behind it (convolution, norm apply) on the same stream; the lap's fill is enqueued on
    that stream too, so it is ordered behind every earlier consumer."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    need = STAT_SLOTS * n * cout * 2
    with _STAT_LOCK:
        ring = _STAT_RINGS.get(key)
        if ring is None or ring[0].numel() < 8 * need:
            ring = [torch.zeros(max(4 << 20, 8 * need), dtype=torch.float64, device=device), 0]
            _STAT_RINGS[key] = ring
        if ring[1] + need > ring[0].numel():
            ring[0].zero_()
            ring[1] = 0
        t = ring[0][ring[1]:ring[1] + need].view(STAT_SLOTS, n, cout, 2)
        ring[1] += need
    return t


def _conv_fwd_stats(x1, x2, wt, stride, want_stats):
    """Forward launch over one or two inputs (virtual concatenation); optionally also the InstanceNorm statistics of the result,
    accumulated in the kernel's epilogue: want_stats = True / "slots" -> double [STAT_SLOTS][N][Cout][2], "tiles" -> the per-tile partials
    float32 [N][tiles][Cout][2] (kept for their tests)."""
    n, h, w, _ = x1.shape
    cout = wt.shape[1]
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x1.device)
    slots = tiles = None
    if want_stats == "tiles":
        tiles = torch.empty((n, _native.lib().octa_conv_stat_tiles(ho, wo), cout, 2), dtype=torch.float32, device=x1.device)
    elif want_stats:
        slots = _stat_slots(x1.device, n, cout)
    _conv3x3_fwd(x1, wt, y, x2=x2, stride=stride, stat_partials=tiles, stat_slots=slots)
    return y, (slots if slots is not None else tiles)


# ---- autograd bindings ---------------------------------------------------------------------------------------------

# A/B switch (development aid): cleared, the mailbox is never armed and autograd adds the two skip gradients itself.
USE_SKIP_GRAD_FUSION = True


class SkipGradMailbox:
    """A tensor with two consumers in the U-Net (a skip connection: the next encoder block and the decoder's concatenation)
    receives two gradients that autograd would add in a separate pass over the tensor (`add<bf16>`: 0.32 ms of the step for the
    four skips). The decoder's gradient is always computed first (everything the encoder block feeds lies between them), so the
    decoder's backward POSTS its gradient here and reports None to autograd, and the encoder convolution's backward adds it in the
    epilogue of its data-gradient launch. One mailbox per skip tensor and forward pass (models/networks.py builds them)."""
    __slots__ = ("pending", "armed")

    def __init__(self):
        self.pending = None
        self.armed = False       # set by the encoder convolution's forward when its backward will collect the posting


class _Conv3x3NHWC(torch.autograd.Function):
    """y = conv3x3(x, weight), padding 1, stride 1 or 2. x [N,H,W,Cin] bf16 (Cin padded to 32 internally),
    weight [Cout,Cin,3,3] (any float dtype; master copy), y [N,Ho,Wo,Cout] bf16."""

    @staticmethod
    def forward(ctx, x, weight, stride, want_stats=False, mailbox=None):
        cin = weight.shape[1]
        ctx.mailbox = None
        ctx.set_materialize_grads(False)      # the statistics output is not differentiable: no zero "gradient" of it (a fill launch per layer)
        if mailbox is not None and USE_SKIP_GRAD_FUSION and x.requires_grad and x.shape[-1] % 32 == 0:
            ctx.mailbox = mailbox
            mailbox.armed = True
        xp = _zero_pad(x.contiguous(), 3, _pad32(x.shape[3]))
        y, part = _conv_fwd_stats(xp, None, pack_weight(weight, xp.shape[-1]), stride, want_stats)
        ctx.save_for_backward(xp, weight)
        ctx.stride, ctx.cin = int(stride), cin
        if want_stats:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, _dpart=None):
        xp, weight = ctx.saved_tensors
        if dy is None:
            return None, None, None, None, None
        dy = _bf16c(dy)
        cin, st = ctx.cin, ctx.stride
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if st == 2:
                assert xp.shape[1] % 2 == 0 and xp.shape[2] % 2 == 0, "stride-2 layers need even input sizes"
            res = None
            if ctx.mailbox is not None:
                res, ctx.mailbox.pending = ctx.mailbox.pending, None       # the decoder's gradient of the same tensor, if posted
            wd = pack_weight_dgrad(weight, xp.shape[-1])
            dx = conv3x3_s2t_nhwc(dy, wd, 0x1ff, res) if st == 2 else conv3x3_nhwc(dy, wd, residual=res)
            if xp.shape[-1] != cin:         # channel-padded input: the GAN trains the generator THROUGH the segmentor's first layer
                dx = dx[..., :cin].contiguous()
        elif ctx.mailbox is not None and ctx.mailbox.pending is not None:
            raise RuntimeError("skip gradient posted but the encoder convolution computes no input gradient")
        if ctx.needs_input_grad[1]:
            direct = (lambda g, acc: _wgrad_acc(xp, None, dy, g, acc, st)) if (xp.shape[-1] == cin and (st == 1 or (xp.shape[1] % 2 == 0 and xp.shape[2] % 2 == 0))) else None
            if st == 1:
                dw = _wgrad_to(weight, lambda: conv3x3_nhwc_wgrad(xp, dy)[:, :cin].to(weight.dtype), direct)
            else:
                dw = _wgrad_to(weight, lambda: _s2_wgrad(xp, dy)[:, :cin].to(weight.dtype), direct)
        return dx, dw, None, None, None


class _Conv3x3ReflectNHWC(torch.autograd.Function):
    """nn.ReflectionPad2d(1) + Conv2d(3, padding 0) (the ResNet blocks of the reference's generator, models/networks.py:151-176) in ONE
    launch per pass: the forward and the weight-gradient kernels mirror the image in their halo fetch (no padded tensor, no crop);
    the data gradient is the full (pad 2) convolution of dy with the flipped weights, folded back by the reflection's adjoint."""

    @staticmethod
    def forward(ctx, x, weight, want_stats=False):
        x = x.contiguous()
        n, h, w, cin = x.shape
        cout = weight.shape[0]
        ctx.set_materialize_grads(False)
        y = torch.empty((n, h, w, cout), dtype=torch.bfloat16, device=x.device)
        wt = pack_weight(weight, cin)
        part = _stat_slots(x.device, n, cout) if want_stats else None       # InstanceNorm statistics from the epilogue (slot form, as conv3x3)
        _native.launch("octa_conv3x3_nhwc_fwd_pad", x.device, x, wt, y, n, h, w, cin, cout, 1, 1, part, STAT_SLOTS if part is not None else 0)
        ctx.save_for_backward(x, weight)
        if want_stats:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, _dpart=None):
        from . import resample
        x, weight = ctx.saved_tensors
        if dy is None:
            return None, None, None
        dy = _bf16c(dy)
        n, h, w, cin = x.shape
        cout = dy.shape[3]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wd = pack_weight_dgrad(weight, cin)
            dxp = torch.empty((n, h + 2, w + 2, cin), dtype=torch.bfloat16, device=x.device)
            _native.launch("octa_conv3x3_nhwc_fwd_pad", x.device, dy, wd, dxp, n, h, w, cout, cin, 2, 0, None, 0)
            dx = torch.empty_like(x)
            resample._launch("octa_reflect_pad_bwd", dxp, dx, n, h, w, cin, 1)
        if ctx.needs_input_grad[1]:
            def wgrad_pad(d_dw, out_mode):
                _native.launch("octa_conv3x3_nhwc_wgrad_pad", x.device, x, dy, d_dw, n, h, w, cin, cout, 1, 1, out_mode)

            def wg():
                dwf = torch.empty((9, cout, cin), dtype=torch.float32, device=x.device)
                wgrad_pad(dwf, _native.WGRAD_TAP_MAJOR)
                return dwf.view(3, 3, cout, cin).permute(2, 3, 0, 1).to(weight.dtype)

            direct = lambda g, acc: wgrad_pad(g, _native.WGRAD_PARAM_ADD if acc else _native.WGRAD_PARAM_SET)
            dw = _wgrad_to(weight, wg, direct)
        return dx, dw, None


USE_FUSED_REFLECT = True     # module switch (development aid)


def conv3x3_reflect(x, weight, want_stats=False):
    """ReflectionPad2d(1) + 3x3 convolution without padding; x [N,H,W,Cin] bf16 with Cin, Cout multiples of 32. want_stats: returns
    (y, statistics slots for instance_norm_leaky_relu_nhwc(..., partials=)) -- None for the slots where the fused kernel does not apply."""
    if USE_FUSED_REFLECT and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 32 == 0 and weight.shape[0] % 32 == 0 and weight.shape[1] == x.shape[-1]:
        return _Conv3x3ReflectNHWC.apply(x, weight, bool(want_stats))
    from . import resample
    y = conv3x3(resample.reflect_pad(x, 1, "nhwc"), weight, 1)[:, 1:-1, 1:-1, :]
    return (y, None) if want_stats else y


class _Conv3x3C1(torch.autograd.Function):
    """First layer: one input channel. want_stats: also the InstanceNorm statistics of the result in slot form (double
    [STAT_SLOTS][N][Cout][2], accumulated by the kernel's epilogue: the norm needs no statistics pass). The data gradient -- needed when
    the image is itself a network's output: the segmentor behind the generator in the GAN-seg step -- is the C -> 1 streaming kernel of
    csrc/thin_conv.hip with the flipped taps (round 5; until then such an input took the matrix-core kernels with the image zero-padded to
    32 channels: a 757 MB fill + copy in front of the layer and a 32-channel data gradient + slice copy behind it)."""

    @staticmethod
    def forward(ctx, x, weight, want_stats=False):
        x = x.contiguous()
        n, h, w, _ = x.shape
        cout = weight.shape[0]
        ctx.set_materialize_grads(False)
        wf = weight.reshape(cout, 9).float().contiguous()
        y = torch.empty((n, h, w, cout), dtype=torch.bfloat16, device=x.device)
        part = _stat_slots(x.device, n, cout) if want_stats else None
        _native.launch("octa_conv3x3_c1_fwd", x.device, x, wf, y, n, h, w, cout, part, STAT_SLOTS if part is not None else 0)
        ctx.save_for_backward(x)
        ctx.w_shape, ctx.w_dtype = weight.shape, weight.dtype
        ctx.weight_ref = weight
        ctx.wf = wf if ctx.needs_input_grad[0] else None        # the taps as the forward used them (fp32 [Cout][9]): the data gradient's weights
        if want_stats:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, _dpart=None):
        (x,) = ctx.saved_tensors
        if dy is None:
            return None, None, None
        dy = _bf16c(dy)
        n, h, w, _ = x.shape
        cout = dy.shape[3]
        def wg():
            dw = torch.empty((cout, 9), dtype=torch.float32, device=x.device)
            _native.launch("octa_conv3x3_c1_wgrad", x.device, x, dy, dw, n, h, w, cout)
            return dw.view(ctx.w_shape).to(ctx.w_dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            # dx[n][y][x] = sum_co sum_t dy[n][y + 1 - ky][x + 1 - kx][co] * w[co][t]: the C -> 1 convolution of dy with the flipped kernel, pad K - 1 - 1
            dx = torch.empty((n, h, w, 1), dtype=torch.bfloat16, device=x.device)
            _native.launch("octa_thinconv_squeeze", x.device, dy, ctx.wf, None, dx, n, h, w, cout, 3, 1, 1)
        return dx, _wgrad_to(ctx.weight_ref, wg) if ctx.needs_input_grad[1] else None, None


def conv3x3(x, weight, stride=1, want_stats=False, mailbox=None):
    """want_stats: also return the statistics for instance_norm_leaky_relu_nhwc(..., partials=)."""
    if x.shape[-1] == 1 and weight.shape[1] == 1 and stride == 1 and weight.shape[0] in (8, 16, 32, 64) and x.shape[2] <= 3840:
        if want_stats == "tiles":                        # the per-tile form belongs to the MFMA kernel: the norm runs its own statistics pass
            return _Conv3x3C1.apply(x, weight, False), None
        return _Conv3x3C1.apply(x, weight, bool(want_stats))          # streaming first-layer kernels
    return _Conv3x3NHWC.apply(x, weight, stride, want_stats, mailbox)


class _Conv3x3CatNHWC(torch.autograd.Function):
    """y = conv3x3(cat(x1, x2, channel axis), weight), stride 1, without materialising the concatenation: the
    kernels read the two tensors as one virtual input and the data gradient is written straight into two tensors
    (MONAI UnetUpBlock: conv_block(torch.cat((transp_conv(x), skip), 1)))."""

    @staticmethod
    def forward(ctx, x1, x2, weight, want_stats=False, mailbox=None):
        ctx.set_materialize_grads(False)
        ctx.mailbox = mailbox if (mailbox is not None and mailbox.armed) else None
        x1, x2 = x1.contiguous(), x2.contiguous()
        c1, c2 = x1.shape[3], x2.shape[3]
        assert x2.shape[:3] == x1.shape[:3] and weight.shape[1] == c1 + c2 and c1 % 32 == 0 and c2 % 32 == 0
        y, part = _conv_fwd_stats(x1, x2, pack_weight(weight), 1, want_stats)
        ctx.save_for_backward(x1, x2, weight)
        if want_stats:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, _dpart=None):
        x1, x2, weight = ctx.saved_tensors
        if dy is None:
            return None, None, None, None, None
        dy = _bf16c(dy)
        dx1 = dx2 = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
            _conv3x3_fwd(dy, pack_weight_dgrad(weight), dx1, y2=dx2, what="octa_conv3x3_nhwc_fwd (data gradient)")
        if ctx.needs_input_grad[2]:
            dw = _wgrad_to(weight, lambda: _conv3x3_wgrad(x1, dy, x2).to(weight.dtype), lambda g, acc: _wgrad_acc(x1, x2, dy, g, acc))
        if ctx.mailbox is not None and dx2 is not None and ctx.needs_input_grad[1]:
            assert ctx.mailbox.pending is None
            ctx.mailbox.pending, dx2 = dx2, None          # collected by the encoder convolution's data-gradient epilogue
        return dx1, dx2, dw, None, None


def conv3x3_cat(x1, x2, weight, want_stats=False, mailbox=None):
    return _Conv3x3CatNHWC.apply(x1, x2, weight, want_stats, mailbox)


class _InstNormLReLUNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope, eps, partials=None):
        x = x.contiguous()
        assert x.dtype == torch.bfloat16 and x.dim() == 4
        B, C = x.shape[0], x.shape[3]
        hw = x.shape[1] * x.shape[2]
        y = torch.empty_like(x)
        mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        w = weight.float().contiguous() if weight is not None else None
        b = bias.float().contiguous() if bias is not None else None
        slots = partials if partials is not None and partials.dtype == torch.float64 else None      # slot form; float32: per-tile partials
        tiles = partials if slots is None else None
        _native.launch("octa_instnorm_lrelu_nhwc_fwd", x.device, x, y, w, b, mean, rstd, B, C, hw, float(slope), float(eps),
                       tiles, int(tiles.shape[1]) if tiles is not None else 0, slots, int(slots.shape[0]) if slots is not None else 0)
        ctx.save_for_backward(x, w, b, mean, rstd)
        ctx.slope, ctx.has_w, ctx.has_b = float(slope), weight is not None, bias is not None
        ctx.w_dtype = weight.dtype if weight is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd = ctx.saved_tensors
        dy = _bf16c(dy)
        B, C = x.shape[0], x.shape[3]
        hw = x.shape[1] * x.shape[2]
        dx = torch.empty_like(x)
        if ctx.has_w and ctx.has_b:
            dwb = torch.empty(2 * C, dtype=torch.float32, device=x.device)     # back to back: the C side clears both with one fill
            dw, db = dwb[:C], dwb[C:]
        else:
            dw = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_w else None
            db = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_b else None
        _native.launch("octa_instnorm_lrelu_nhwc_bwd", x.device, x, dy, w, b, mean, rstd, dx, dw, db, B, C, hw, ctx.slope)
        return dx, (dw.to(ctx.w_dtype) if dw is not None else None), (db.to(ctx.w_dtype) if db is not None else None), None, None, None


def instance_norm_leaky_relu_nhwc(x, weight, bias, negative_slope=0.01, eps=1e-5, partials=None):
    """partials: per-tile statistics produced by the convolution that wrote x (conv3x3(..., want_stats=True))."""
    return _InstNormLReLUNHWC.apply(x, weight, bias, negative_slope, eps, partials)


def _s2_wgrad(x_big, dy_small, taps2=((0, 1, 2), (0, 1, 2))):
    """Weight gradient [Cout, Cin, 3, 3] (float32) of a stride-2, padding-1 3x3 conv with input x_big [N,2H,2W,Cin] and
    output gradient dy_small [N,H,W,Cout]; taps2 = the (r, s) taps that are wanted (others come back zero)."""
    x_big, dy_small = x_big.contiguous(), dy_small.contiguous()
    mask = 0
    for r in taps2[0]:
        for s_ in taps2[1]:
            mask |= 1 << (3 * r + s_)
    return _conv3x3_wgrad(x_big, dy_small, stride=2, tap_mask=mask)


class _ConvT2x2NHWC(torch.autograd.Function):
    """ConvTranspose2d(kernel 2, stride 2, no bias) as the ADJOINT of a stride-2 3x3 convolution whose taps r, s = 0
    are zero: forward = that convolution's data-gradient kernel (virtual zero insertion), backward = its forward
    kernel (stride 2) and its weight gradient -- all on the MFMA kernels, no GEMM + pixel-shuffle round trip."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous()
        # the 3x3 form wc has taps r, s in {1, 2}; flipped for the data-gradient form they sit at r, s in {0, 1}
        y = conv3x3_s2t_nhwc(x, pack_convt2x2(weight)[1], 0b000011011)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _bf16c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = conv3x3_nhwc(dy, pack_convt2x2(weight)[0], stride=2, tap_mask=0b110110000)
        if ctx.needs_input_grad[1]:
            dw = _wgrad_to(weight, lambda: _s2_wgrad(dy, x, taps2=((1, 2), (1, 2)))[:, :, 1:, 1:].to(weight.dtype))
        return dx, dw


# The 1x1 "transposed" layer at the U-Net's bottleneck (512 -> 256 at 152^2) runs the repository's own MFMA convolution with only the centre
# tap unmasked: no vendor kernel is left in the training step. (Round 3's route through hipBLASLt -- plain GEMMs through torch, the weight
# gradient split by hand into batched products; 1.4 % faster on the whole step -- left the product in round 6: tools/micro/try_bmm_splitk.py
# keeps the measurement.)


def _t1x1_packs(weight):
    """[9][Cout][Cin] bf16 operands of the tap-masked 3x3 kernel for a ConvTranspose2d(k = 1) weight [Cin, Cout, 1, 1]: forward
    (tap 4 = W^T) and data gradient (tap 4 = W); the masked taps are never fetched. Cached on the parameter (weight_cache.cached).
    They equal fwd_layout / dgrad_layout of the 3x3 weight whose centre tap is W^T; the centre tap is written directly because it needs
    no flip: that route would add a torch launch per layer to every optimiser step."""
    def make():
        cin, cout = weight.shape[0], weight.shape[1]
        wm = weight.detach().reshape(cin, cout).to(torch.bfloat16)
        fwd = torch.zeros((9, cout, cin), dtype=torch.bfloat16, device=weight.device)
        dg = torch.zeros((9, cin, cout), dtype=torch.bfloat16, device=weight.device)
        fwd[4] = wm.t()
        dg[4] = wm
        return slice_major(fwd), slice_major(dg)
    return weight_cache.cached(weight, "_octa_convt1x1", None, make)


class _ConvT1x1NHWC(torch.autograd.Function):
    """ConvTranspose2d(kernel 1, stride 1, no bias) = a 1x1 convolution with the transposed weight: the MFMA 3x3 kernels with the
    tap mask 0b000010000 (forward, data gradient on the swapped weight, weight gradient), csrc/conv.hip."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous()
        n, h, w, cin = x.shape
        cout = weight.shape[1]
        ctx.w_shape, ctx.w_dtype = weight.shape, weight.dtype
        fwd, dg = _t1x1_packs(weight)
        ctx.save_for_backward(x, dg)
        return conv3x3_nhwc(x, fwd, tap_mask=1 << 4)

    @staticmethod
    def backward(ctx, dy):
        x, wm = ctx.saved_tensors
        dy = _bf16c(dy)
        n, h, w, cin = x.shape
        cout = dy.shape[3]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = conv3x3_nhwc(dy, wm, tap_mask=1 << 4)          # wm: the data-gradient pack [9][Cin][Cout]
        if ctx.needs_input_grad[1]:
            # as a convolution weight [Cout_conv = cout][Cin_conv = cin][3][3] with only tap (1, 1): dW[co][ci] = sum_p dy[p][co] x[p][ci]
            dw = conv3x3_nhwc_wgrad(x, dy, tap_mask=1 << 4)[:, :, 1, 1].t().reshape(ctx.w_shape).to(ctx.w_dtype)
        return dx, dw


def conv_transpose_kxk_nhwc(x, weight, k):
    if k in (1, 2) and x.shape[-1] % 32 == 0 and weight.shape[1] % 32 == 0:
        return (_ConvT2x2NHWC if k == 2 else _ConvT1x1NHWC).apply(x, weight)
    from . import networks
    networks._vendor_fallback("DynUNet transposed convolution (NHWC)", f"k = {k}, {x.shape[-1]} -> {weight.shape[1]} channels: GEMM through hipBLASLt "
                              "(the MFMA kernels need k in (1, 2) and channel counts % 32 == 0)")
    return _conv_transpose_kxk_gemm(x, weight, k)


def _conv_transpose_kxk_gemm(x, weight, k):
    """ConvTranspose2d with kernel == stride == k (no padding, no bias) on NHWC bf16: every input pixel owns a
    disjoint k x k output patch, so it is one GEMM [N*H*W, Cin] x [Cin, k*k*Cout] (hipBLASLt through torch) plus a
    pixel shuffle. weight: the torch parameter [Cin, Cout, k, k]."""
    n, h, w, cin = x.shape
    cout = weight.shape[1]
    wm = weight.permute(0, 2, 3, 1).reshape(cin, k * k * cout).to(torch.bfloat16)
    y = torch.matmul(x.reshape(n * h * w, cin), wm)
    if k == 1:
        return y.view(n, h, w, cout)
    return y.view(n, h, w, k, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, h * k, w * k, cout)


class _Head1NHWC(torch.autograd.Function):
    """1x1 convolution to ONE channel with bias on the streaming HIP kernels (csrc/conv.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        n, h, w, c = x.shape
        wv = weight.reshape(-1).float().contiguous()
        y = torch.empty((n, h, w, 1), dtype=torch.bfloat16, device=x.device)
        bv = bias.float().contiguous() if bias is not None else None      # read on the device: no host round trip in the step
        _native.launch("octa_head1_nhwc_fwd", x.device, x, wv, bv, n * h * w, c, y)
        ctx.save_for_backward(x, wv)
        ctx.w_shape, ctx.w_dtype, ctx.has_bias = weight.shape, weight.dtype, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wv = ctx.saved_tensors
        dy = _bf16c(dy)
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        dw = torch.empty(c, dtype=torch.float32, device=x.device)
        db = torch.empty(1, dtype=torch.float32, device=x.device)
        _native.launch("octa_head1_nhwc_bwd", x.device, x, dy, wv, n * h * w, c, dx, dw, db)
        return dx, dw.view(ctx.w_shape).to(ctx.w_dtype), (db.to(ctx.w_dtype) if ctx.has_bias else None)


class _InstNormLReLUHead1NHWC(torch.autograd.Function):
    """InstanceNorm(affine) + LeakyReLU + 1x1 convolution to one channel (+ bias) in one pair of passes each way
    (csrc/norm.hip octa_instnorm_lrelu_head1_nhwc_*): the normalised tensor and its gradient never reach HBM."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope, eps, head_w, head_b, partials=None):
        x = x.contiguous()
        assert x.dtype == torch.bfloat16 and x.dim() == 4
        B, H, W, C = x.shape
        f32 = dict(dtype=torch.float32, device=x.device)
        g = gamma.float().contiguous() if gamma is not None else None
        bt = beta.float().contiguous() if beta is not None else None
        hw_ = head_w.reshape(-1).float().contiguous()
        hb = head_b.float().contiguous() if head_b is not None else None
        mean, rstd = torch.empty(B * C, **f32), torch.empty(B * C, **f32)
        logits = torch.empty((B, H, W, 1), dtype=torch.bfloat16, device=x.device)
        slots = partials if partials is not None and partials.dtype == torch.float64 else None      # statistics of x from the convolution that wrote it
        _native.launch("octa_instnorm_lrelu_head1_nhwc_fwd", x.device, x, g, bt, hw_, hb, mean, rstd, logits, B, C, H * W, float(slope), float(eps),
                       slots, int(slots.shape[0]) if slots is not None else 0)
        ctx.save_for_backward(x, g, bt, hw_, mean, rstd)
        ctx.slope = float(slope)
        ctx.meta = (gamma is not None, beta is not None, head_b is not None, head_w.shape, head_w.dtype,
                    gamma.dtype if gamma is not None else None)
        return logits

    @staticmethod
    def backward(ctx, dl):
        x, g, bt, hw_, mean, rstd = ctx.saved_tensors
        has_g, has_b, has_hb, hw_shape, hw_dtype, g_dtype = ctx.meta
        dl = _bf16c(dl)
        B, H, W, C = x.shape
        f32 = dict(dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        dgb = torch.empty(2 * C, **f32)                   # back to back: one fill clears both
        dg, db = dgb[:C], dgb[C:]
        dhw, dhb = torch.empty(C, **f32), torch.empty(1, **f32)
        _native.launch("octa_instnorm_lrelu_head1_nhwc_bwd", x.device, x, dl, g, bt, hw_, mean, rstd, dx, dg, db, dhw, dhb, B, C, H * W, ctx.slope)
        return (dx, dg.to(g_dtype) if has_g else None, db.to(g_dtype) if has_b else None, None, None,
                dhw.view(hw_shape).to(hw_dtype), dhb.to(hw_dtype) if has_hb else None, None)


def norm_lrelu_head1_ok(c, head_weight):
    return head_weight.shape[0] == 1 and head_weight.shape[1] == c and c in (8, 16, 32, 64, 128, 256)


def instance_norm_leaky_relu_head1_nhwc(x, gamma, beta, negative_slope, eps, head_weight, head_bias, partials=None):
    """x [N,H,W,C] bf16 (raw convolution output) -> logits [N,H,W,1] bf16 = head(lrelu(instance_norm(x))). partials: the slot-form
    statistics of x from the convolution that wrote it (conv3x3(..., want_stats=True))."""
    return _InstNormLReLUHead1NHWC.apply(x, gamma, beta, negative_slope, eps, head_weight, head_bias, partials)


class _HeadNNHWC(torch.autograd.Function):
    """1x1 convolution to 2..64 channels with bias on the matrix cores (csrc/head.hip): NHWC in, CHANNEL-FIRST [N, Cout, H, W] out."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        n, h, w, c = x.shape
        cout = weight.shape[0]
        wv = weight.reshape(cout, c).float().contiguous()
        bv = bias.float().contiguous() if bias is not None else None
        y = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=x.device)
        _native.launch("octa_headn_nhwc_fwd", x.device, x, wv, bv, n, h * w, c, cout, y)
        ctx.save_for_backward(x, wv)
        ctx.w_shape, ctx.w_dtype, ctx.has_bias = weight.shape, weight.dtype, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wv = ctx.saved_tensors
        dy = _bf16c(dy)
        n, h, w, c = x.shape
        cout = wv.shape[0]
        dx = torch.empty_like(x)
        dw = torch.empty((cout, c), dtype=torch.float32, device=x.device)
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
        _native.launch("octa_headn_nhwc_bwd", x.device, x, dy, wv, n, h * w, c, cout, dx, dw, db)
        return dx, dw.view(ctx.w_shape).to(ctx.w_dtype), (db.to(ctx.w_dtype) if ctx.has_bias else None)


def headn_ok(cin, weight):
    """The matrix-core head applies (and conv1x1_bias_nhwc's result is channel-first). Inside networks.vendor_reference() the old GEMM is
    wanted: the reference side of the head's parity test."""
    from . import networks
    return cin in (32, 64) and 2 <= weight.shape[0] <= 64 and weight.shape[1] == cin and networks._REFERENCE_DEPTH[0] == 0


def conv1x1_bias_nhwc(x, weight, bias):
    """1x1 convolution head: weight [Cout, Cin, 1, 1], bias [Cout]. One output channel -> [N,H,W,1] bf16 (streaming kernels); 2..64
    output channels from 32 or 64 -> CHANNEL-FIRST contiguous [N,Cout,H,W] bf16 (csrc/head.hip: what the loss and the post-processing
    read); any other shape -> [N,H,W,Cout] bf16 through the vendor GEMM (an error under OCTA_STRICT=1)."""
    if weight.shape[0] == 1 and x.shape[-1] % 8 == 0 and x.shape[-1] <= 256 and 256 % (x.shape[-1] // 8) == 0:
        return _Head1NHWC.apply(x, weight, bias)
    if x.dtype == torch.bfloat16 and headn_ok(x.shape[-1], weight):
        return _HeadNNHWC.apply(x, weight, bias)
    from . import networks
    networks._vendor_fallback("DynUNet output block (NHWC)", f"{x.shape[-1]} -> {weight.shape[0]} channels: GEMM through hipBLASLt (the streaming head covers one output "
                              "channel, the matrix-core head 2..64 channels from 32 or 64)")
    n, h, w, cin = x.shape
    y = torch.matmul(x.reshape(n * h * w, cin), weight.reshape(weight.shape[0], cin).t().to(torch.bfloat16))
    if bias is not None:
        y = y + bias.to(torch.bfloat16)
    return y.view(n, h, w, weight.shape[0])


# ---- normalise-on-load path: the normalised activations never go to HBM ---------------------------------------------
# A "lazy" activation is a triple (t, scale, shift): t aliases the RAW output of a convolution, and every consumer reads
# it as lrelu(t * scale + shift). For autograd t IS the normalised activation: the convolutions return dL/d(normalised)
# for it, contributions of several consumers are summed by autograd, and _LazyNorm.backward turns the sum into the
# gradient of the raw tensor with the usual InstanceNorm+LeakyReLU backward kernels.

LRELU_SLOPE = 0.01


class _LazyNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, slope, eps):
        x = x.contiguous()
        B, C = x.shape[0], x.shape[3]
        hw = x.shape[1] * x.shape[2]
        f32 = dict(dtype=torch.float32, device=x.device)
        mean, rstd, scale, shift = (torch.empty(B * C, **f32) for _ in range(4))
        w = weight.float().contiguous() if weight is not None else None
        b = bias.float().contiguous() if bias is not None else None
        _native.launch("octa_instnorm_nhwc_stats", x.device, x, w, b, mean, rstd, scale, shift, B, C, hw, float(eps))
        ctx.save_for_backward(x, w, b, mean, rstd)
        ctx.slope, ctx.has_w, ctx.has_b = float(slope), weight is not None, bias is not None
        ctx.w_dtype = weight.dtype if weight is not None else None
        y = x.view(x.shape)          # same storage: consumers apply scale / shift / LeakyReLU while loading
        ctx.mark_non_differentiable(scale, shift)
        return y, scale, shift

    @staticmethod
    def backward(ctx, dy, _ds, _dh):
        return _InstNormLReLUNHWC.backward(ctx, dy)[:5]


def lazy_norm(x, weight, bias, negative_slope=LRELU_SLOPE, eps=1e-5):
    """-> (t, scale, shift): see the section comment."""
    return _LazyNorm.apply(x, weight, bias, negative_slope, eps)


class _Materialise(torch.autograd.Function):
    """y = lrelu(t * scale + shift) as a real tensor, for the consumers that are not normalise-on-load kernels."""

    @staticmethod
    def forward(ctx, t, scale, shift, slope):
        t = t.contiguous()
        y = torch.empty_like(t)
        B, C = t.shape[0], t.shape[3]
        _native.launch("octa_scale_shift_lrelu_nhwc", t.device, t, y, scale, shift, B, C, t.shape[1] * t.shape[2], float(slope))
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None, None      # t stands for the normalised activation in the graph


def materialise(lazy, slope=LRELU_SLOPE):
    t, sc, sh = lazy
    return t if sc is None else _Materialise.apply(t, sc, sh, slope)


class _ConvLazy(torch.autograd.Function):
    """conv3x3 over one or two (virtually concatenated) lazy inputs, stride 1 or 2 (stride 2: single input)."""

    @staticmethod
    def forward(ctx, x1, sc1, sh1, x2, sc2, sh2, weight, stride, slope):
        x1 = x1.contiguous()
        n, h, w, c1 = x1.shape
        c2 = 0
        if x2 is not None:
            x2 = x2.contiguous()
            c2 = x2.shape[3]
        cin, cout = c1 + c2, weight.shape[0]
        assert weight.shape[1] == cin and c1 % 32 == 0 and c2 % 32 == 0 and cout % 32 == 0
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        y = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x1.device)
        _conv3x3_fwd(x1, pack_weight(weight), y, x2=x2, stride=stride, norm=(sc1, sh1, sc2, sh2), slope=slope)
        ctx.save_for_backward(x1, sc1, sh1, x2, sc2, sh2, weight)
        ctx.stride, ctx.slope = int(stride), float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, sc1, sh1, x2, sc2, sh2, weight = ctx.saved_tensors
        dy = _bf16c(dy)
        st = ctx.stride
        dx1 = dx2 = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[3]:
            dx1 = torch.empty_like(x1)
            dx2 = torch.empty_like(x2) if x2 is not None else None
            _conv3x3_fwd(dy, pack_weight_dgrad(weight), dx1, y2=dx2, in_dilation=st, what="octa_conv3x3_nhwc_fwd (data gradient)")
        if ctx.needs_input_grad[6]:
            if st == 1:
                dw = _conv3x3_wgrad(x1, dy, x2, norm=(sc1, sh1, sc2, sh2), slope=ctx.slope).to(weight.dtype)
            else:
                xm = x1 if sc1 is None else _Materialise.apply(x1, sc1, sh1, ctx.slope)   # parity planes need the tensor itself
                dw = _s2_wgrad(xm, dy).to(weight.dtype)
        return dx1, None, None, dx2, None, None, dw, None, None


def conv3x3_lazy(a, weight, stride=1, b=None, slope=LRELU_SLOPE):
    """a, b: lazy activations (t, scale, shift) (scale None = plain tensor); b is virtually concatenated after a."""
    t2, s2, h2 = b if b is not None else (None, None, None)
    return _ConvLazy.apply(a[0], a[1], a[2], t2, s2, h2, weight, stride, slope)


# ---- 4x4 stride-1 convolution (PatchGAN inner layers) -----------------------------------------------------------------

def conv4x4_nhwc(x, wt, pad):
    """x [N,H,W,Cin] bf16, wt [16,Cout,Cin] bf16 (tap 4r+s) -> [N,H+2pad-3,W+2pad-3,Cout] bf16 (csrc/conv.hip, KS = 4)."""
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and wt.dtype == torch.bfloat16 and wt.is_contiguous()
    n, h, w, cin = x.shape
    cout = wt.shape[1]
    y = torch.empty((n, h + 2 * pad - 3, w + 2 * pad - 3, cout), dtype=torch.bfloat16, device=x.device)
    _native.launch("octa_conv4x4_nhwc_fwd", x.device, x, wt, y, n, h, w, cin, cout, int(pad))
    return y


class _Conv4x4NHWC(torch.autograd.Function):
    """Conv2d(Cin, Cout, 4, stride 1, padding 1) without bias on NHWC bf16: forward, data gradient and weight gradient on
    the K = 4 instantiations of the MFMA kernels (the weight gradient holds 16 accumulator tiles = 256 AGPRs per wave)."""

    @staticmethod
    def forward(ctx, x, weight):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        return conv4x4_nhwc(x, pack_weight(weight), 1)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _bf16c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # dx = full correlation of dy with the flipped kernel, channels transposed: padding 3 - 1 = 2
            dx = conv4x4_nhwc(dy, pack_weight_dgrad(weight), 2)
        if ctx.needs_input_grad[1]:
            n, h, w, cin = x.shape
            cout = dy.shape[3]

            def wg():
                d = torch.empty((16, cout, cin), dtype=torch.float32, device=x.device)
                _native.launch("octa_conv4x4_nhwc_wgrad", x.device, x, dy, d, n, h, w, cin, cout)
                return d.view(4, 4, cout, cin).permute(2, 3, 0, 1).to(weight.dtype)
            dw = _wgrad_to(weight, wg)
        return dx, dw


def conv4x4(x, weight):
    """weight: the torch parameter [Cout, Cin, 4, 4]; stride 1, padding 1, no bias."""
    return _Conv4x4NHWC.apply(x, weight)
