"""The noise-model kernels of csrc/augment.hip on the device. octa_speckle_brightness against the float64 reference and the derived bound
of tests/_speckle_ref.py (proved on the CPU by tests/test_speckle_ref.py), with its exact claims: every image's minimum exactly 0, no
NaN, equal bits on a second run. octa_background_noise, which has no rounding to allow for, exactly equal to
torch.maximum(img.double(), noise.double() * u) and to its .float(), both outputs from one launch, a NaN of img coming through. Outputs
lie between sentinels; every test prints its error / bound ratios before it asserts them.

Largest error / bound measured on an MI355X, on the kernels of commit c9efa0d, which the commit that adds this file leaves as they are:
    speckle 0.068 (3 x 33 x 257, isolation); every image's minimum 0, no NaN; background noise: 0 differing elements for every n"""
import pytest
import torch

import _speckle_ref as S
from _guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = lambda s: "x".join(map(str, s))


def _speckle(img, grid9, u):
    """the entry point itself, twice, into sentinel-guarded buffers"""
    from octa_autosegmentation_amd import _native
    B, H, W = img.shape
    outs = []
    for _ in range(2):
        g = Guarded((B, H, W), torch.float32)
        mm = torch.full((B + 2, 2), 0x5A5B5C5D, dtype=torch.int32, device=DEV)          # one sentinel row in front, one behind
        _native.launch("octa_speckle_brightness", img.device, img, grid9, u, B, H, W, g.t, mm[1:B + 1])
        torch.cuda.synchronize()
        assert g.intact() and g.unwritten() == 0 and bool((mm[0] == 0x5A5B5C5D).all()) and bool((mm[B + 1] == 0x5A5B5C5D).all())
        outs.append(g.t.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    return outs[0]


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_speckle_brightness(hip_lib_built, shape):
    from octa_autosegmentation_amd.data import gpu_augment
    rat = {}
    for name, img, grid9, u in S.cases(shape):
        img, grid9, u = img.to(DEV), grid9.to(DEV), u.to(DEV)
        ref, tol = S.reference(img, grid9, u)
        got = _speckle(img, grid9, u)
        rat[name] = S.ratio(got, ref, tol)
        print("SPECKLE", shape, name, "minimum of each image", got.amin((1, 2)).tolist(), "NaN", int(torch.isnan(got).sum()))
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got.amin((1, 2)), torch.zeros(shape[0], device=DEV)), name
        assert torch.equal(gpu_augment.speckle_brightness(img, grid9, u), got)
    print("RATIO speckle", shape, {k: float(f"{v:.4g}") for k, v in rat.items()})
    assert all(v <= 1.0 for v in rat.values()), rat


def _same(got, want):
    """equal values, and NaN exactly where the reference has NaN"""
    return bool((torch.isnan(got) == torch.isnan(want)).all()) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2310])
def test_background_noise_is_exact(hip_lib_built, n):
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.data import gpu_augment
    g = torch.Generator().manual_seed(n)
    img, noise = torch.rand(n, generator=g), torch.rand(n, generator=g)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    img[::7], noise[::14] = 0.0, 0.0                    # zeros against zeros at every 14th element: ties
    noise[3::7] = img[3::7]
    u[3::14] = 1.0                                      # and ties of nonzero values
    if n > 1:
        img[n // 2] = float("nan")
    img, noise, u = img.to(DEV), noise.to(DEV), u.to(DEV)
    want = torch.maximum(img.double(), noise.double() * u)
    assert int(torch.isnan(want).sum()) == (1 if n > 1 else 0) and bool((img.double() == noise.double() * u).any())
    outs = []
    for _ in range(2):
        o64, o32 = Guarded((n,), torch.float64), Guarded((n,), torch.float32)
        _native.launch("octa_background_noise", img.device, img, noise, u, n, o64.t, o32.t)          # both outputs from one launch
        torch.cuda.synchronize()
        assert o64.intact() and o32.intact() and o64.unwritten() == 0 and o32.unwritten() == 0
        outs.append((o64.t.clone(), o32.t.clone()))
    assert torch.equal(outs[0][0].view(torch.int64), outs[1][0].view(torch.int64)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    print("BACKGROUND", n, "differing float64", int((torch.nan_to_num(outs[0][0]) != torch.nan_to_num(want)).sum()),
          "differing float32", int((torch.nan_to_num(outs[0][1]) != torch.nan_to_num(want.float())).sum()))
    assert _same(outs[0][0], want) and _same(outs[0][1], want.float())
    # one output at a time, as the wrapper asks for them
    assert _same(gpu_augment.background_noise(img, noise, u), want) and _same(gpu_augment.background_noise(img, noise, u, torch.float32), want.float())


def test_background_noise_refuses_bad_arguments(hip_lib_built):
    from octa_autosegmentation_amd import _native
    x = torch.rand(16, device=DEV)
    u = torch.rand(16, device=DEV, dtype=torch.float64)
    o64, o32 = Guarded((16,), torch.float64), Guarded((16,), torch.float32)
    lib, ctx, stream = _native.lib(), _native.ctx(torch.device(DEV).index), _native.current_stream_ptr()
    good = [x.data_ptr(), x.data_ptr(), u.data_ptr(), 16, o64.t.data_ptr(), o32.t.data_ptr()]

    def bad(*pairs):
        a = list(good)
        for i, v in pairs:
            a[i] = v
        return a

    for args in (bad((4, None), (5, None)), bad((3, 0)), bad((3, -1)), bad((0, None)), bad((1, None)), bad((2, None))):
        assert lib.octa_background_noise(ctx, *args, stream) == -2
        assert lib.octa_last_error().decode() == "octa_background_noise: bad arguments"
    assert lib.octa_background_noise(None, *good, stream) == -2
    with pytest.raises(_native.OctaHipError):
        _native.launch("octa_background_noise", x.device, x, x, u, 0, o64.t, o32.t)
    torch.cuda.synchronize()
    assert o64.untouched() and o32.untouched()
