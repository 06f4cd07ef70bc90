"""GPU: the six kernels of csrc/blur.hip against the float64 references of tests/_blur_ref.py (proved on the CPU by tests/test_blur_ref.py).
Direct calls of the entry points through _native.launch, every output between sentinels: exact cases bit for bit in both dtypes and both
layouts, real-valued cases inside the derived bound on every element (the reflection pad's forward is a copy: bit for bit), the impulse
matrices of forward and backward bit for bit against each other and the reference at every border configuration of a short axis, the three
forms of the dispatch (fp32 scalar, bf16 scalar, bf16 with 8 channels per thread) against each other bit for bit, and the refusals.
Every test prints its error / bound ratios before it asserts them. A GPU error ends the session (pytest.exit).

MEASURED on the MI355X, on the kernels as the commit that adds this file found them (csrc/blur.hip is unchanged). Every exact case and every
impulse matrix: 0 differing elements. Largest error / bound of the real-valued cases (the CPU emulation of tests/test_blur_ref.py in
brackets; the bf16 figures are the half ulp, which a value just above a power of two uses in full):
              pad bwd        down fwd       down bwd       up fwd         up bwd
    fp32      0.314 (0.314)  0.465 (0.465)  0.192 (0.192)  0.805 (0.805)  0.247 (0.247)
    bf16      0.996 (0.996)  0.996 (0.996)  0.996 (0.996)  0.996 (0.996)  0.988 (0.988)
The pad's forward is a copy: 0 differing elements in both dtypes. The fp32 figures equal the emulation's to every printed digit.
"""
import pytest
import torch

import _blur_ref as br
from _guarded import DEV, Guarded

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = {F32: 0, BF: 1}
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a faulted device: start nothing more on it
        pytest.exit(f"GPU error, session ended: {e}", returncode=3)


def _run(op, v, H, W, pad, layout="nhwc", in_off=0, out_off=0):
    """v: planes [B][h][w][C] on the device, in the dtype the kernel gets -> (result as planes [B][ho][wo][C], its Guarded). nchw: the same
    data as B * C planes of one channel. in_off / out_off: element offsets of the two tensors from a 16-byte-aligned address."""
    from octa_autosegmentation_amd import _native
    B, h, w, C = v.shape
    ho, wo = br.out_hw(op, H, W, pad) if op.endswith("fwd") else (H, W)
    src = Guarded((B, C, h, w) if layout == "nchw" else (B, h, w, C), v.dtype, offset=in_off)
    src.t.copy_(v.permute(0, 3, 1, 2) if layout == "nchw" else v)
    out = Guarded((B, C, ho, wo) if layout == "nchw" else (B, ho, wo, C), v.dtype, offset=out_off)
    assert src.t.data_ptr() % 16 == in_off * v.element_size() % 16 and out.t.data_ptr() % 16 == out_off * v.element_size() % 16
    b, c = (B * C, 1) if layout == "nchw" else (B, C)
    _native.launch(br.ENTRY[op], v.device, src.t, out.t, DTYPES[v.dtype], b, H, W, c, *((pad,) if op.startswith("pad") else ()))
    _sync()
    assert out.intact() and src.intact(), f"{op}: a sentinel around a buffer was overwritten"
    assert out.unwritten() == 0, f"{op}: {out.unwritten()} elements were never stored"
    assert torch.equal(src.t, v.permute(0, 3, 1, 2) if layout == "nchw" else v), f"{op}: the kernel's input changed"
    return (out.t.permute(0, 2, 3, 1) if layout == "nchw" else out.t), out


WORST = {}


@pytest.mark.parametrize("shape", br.SHAPES + br.DISPATCH_SHAPES, ids=IDS)
@pytest.mark.parametrize("op", br.OPS)
def test_cases(hip_lib_built, op, shape):
    """exact: one legal result; real-valued: the per-element bound; fp32 and bf16, planes of one channel (NCHW) and channels last"""
    B, C, H, W = shape
    rat = {}
    for var in ("exact", "real"):
        pad = (br.exact_pad(shape) if var == "exact" else br.PADS.get(shape, 1)) if op.startswith("pad") else 0
        v0 = br.case(op, shape, var, pad).to(DEV)
        for dtype in (F32, BF):
            v = v0.to(dtype)
            ref, S = br.ref_of(op, v, H, W, pad, var)
            for layout in ("nchw", "nhwc"):
                got, _ = _run(op, v, H, W, pad, layout)
                key = f"{var} {'bf16' if dtype == BF else 'fp32'} {layout}"
                assert got.dtype == dtype and got.shape == ref.shape
                if var == "exact" or op == "pad_fwd":
                    rat[key] = 0.0 if torch.equal(got.double(), ref) else float("inf")
                else:
                    rat[key] = br.ratio(got, ref, br.tolerance(op, ref, S, dtype == BF))
                    k = (op, "bf16" if dtype == BF else "fp32")
                    WORST[k] = max(WORST.get(k, 0.0), rat[key])
    print("RATIO", op, shape, {k: float(f"{v:.4g}") for k, v in rat.items()}, "D", br.D[op])
    print("WORST so far", {f"{a} {b}": float(f"{v:.4g}") for (a, b), v in WORST.items()})
    bad = {k: v for k, v in rat.items() if not v <= 1.0}
    assert not bad, f"{op} {shape}: error / bound above 1 (exact: not the one legal result) for {bad}"


@pytest.mark.parametrize("kind", ["pad", "down", "up"])
def test_impulse_matrices_bit_for_bit(hip_lib_built, kind):
    """Forward and backward operator on all unit impulses times 16, impulses along the plane axis (fp32 and bf16) and along the channel axis
    (bf16: the 8-channel form where their number is a multiple of 8): the backward's matrix is the exact transpose of the forward's and
    both are the reference's 16 A_y (x) A_x -- every tap of pad_sources, down_taps and up_taps at pad = H - 1, H = 2, odd H, replicated borders."""
    sets = [(h, w, p) for h, w in br.IMPULSE_HW for p in (range(1, min(h, w)) if kind == "pad" else (0,))]
    if kind == "up":
        sets += [(h, w, 0) for h, w in br.IMPULSE_UP_EXTRA]
    differing = 0
    for H, W, pad in sets:
        mats = {}
        for way in ("fwd", "bwd"):
            op = f"{kind}_{way}"
            h, w = br.in_hw(op, H, W, pad)
            want = br.impulse_reference(op, H, W, pad).to(DEV)
            eye = 16.0 * torch.eye(h * w, device=DEV)
            for dtype in (F32, BF):
                got, _ = _run(op, eye.view(h * w, h, w, 1).to(dtype), H, W, pad)                      # impulse i in plane i
                m = got.reshape(h * w, -1).double()
                differing += int((m != want).sum())
                assert torch.equal(m, want), (op, H, W, pad, dtype, "planes")
            got, _ = _run(op, eye.t().reshape(1, h, w, h * w).to(BF), H, W, pad)                      # impulse i in channel i
            mc = got.reshape(-1, h * w).t().double()
            differing += int((mc != want).sum())
            assert torch.equal(mc, want), (op, H, W, pad, "channels", (h * w) % 8)
            mats[way] = m
        assert torch.equal(mats["fwd"], mats["bwd"].t()), (kind, H, W, pad)
    print("IMPULSE", kind, len(sets), "configurations, differing entries", differing)


@pytest.mark.parametrize("shape", br.DISPATCH_SHAPES, ids=IDS)
@pytest.mark.parametrize("op", br.OPS)
def test_dispatch_forms_agree_bit_for_bit(hip_lib_built, op, shape):
    """bf16, channels last, real-valued data. C in {8, 24}: 16-byte-aligned pointers run 8 channels per thread; the same data 2 bytes further
    (input and output) runs the scalar form with C % 8 == 0; C = 12 runs the scalar form at an aligned address. All of them, and the run on
    planes of one channel (NCHW), give the same bits; an offset of the input alone or of the output alone does too."""
    B, C, H, W = shape
    pad = br.PADS.get(shape, 1) if op.startswith("pad") else 0
    v = br.case(op, shape, "real", pad).to(DEV).to(BF)
    ref, S = br.ref_of(op, v, H, W, pad, "real")
    base, _ = _run(op, v, H, W, pad, "nhwc")
    q = br.ratio(base, ref, br.tolerance(op, ref, S, True)) if op != "pad_fwd" else (0.0 if torch.equal(base.double(), ref) else float("inf"))
    print("RATIO dispatch", op, shape, float(f"{q:.4g}"))
    assert q <= 1.0
    for name, kw in (("both + 2 bytes", dict(in_off=1, out_off=1)), ("input + 2 bytes", dict(in_off=1)), ("output + 2 bytes", dict(out_off=1)),
                     ("both + 8 bytes", dict(in_off=4, out_off=4)), ("nchw", dict(layout="nchw"))):
        other, _ = _run(op, v, H, W, pad, **kw)
        assert torch.equal(other.contiguous().view(torch.int16), base.contiguous().view(torch.int16)), f"{op} {shape}: {name} differs from the aligned run"


@pytest.mark.parametrize("name", list(br.refusals()))
def test_refusals(hip_lib_built, name):
    """each refused call returns an error and leaves the output untouched; the buffers are larger than anything the call could address"""
    from octa_autosegmentation_amd import _native
    fam, dtype, B, H, W, C, pad, alias = br.refusals()[name]
    for op in br.OPS:
        if fam is not None and not op.startswith(fam):
            continue
        tdt = BF if dtype == 1 else F32
        src, out = Guarded((8192,), tdt), Guarded((8192,), tdt)
        with pytest.raises(_native.OctaHipError):
            _native.launch(br.ENTRY[op], out.t.device, out.t if alias else src.t, out.t, dtype, B, H, W, C, *((pad,) if op.startswith("pad") else ()))
        _sync()
        assert out.untouched() and src.untouched(), f"{name}: the refused {op} wrote"
