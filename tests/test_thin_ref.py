"""Proves tests/_thin_ref.py without a GPU: an emulation of the arithmetic of csrc/thin_conv.hip in torch on the CPU (fp32 conv2d and sums
on the bf16-rounded operands, one rounding to bf16) reproduces every exact case bit for bit and stays inside the bound of every
real-valued case that tests/test_thin_conv_gpu.py runs, and each of a list of wrong kernels (mutants of the emulation) is rejected by at
least one named case. Also: whatever models/thin_conv.supported() admits is a shape the native entry points accept, by a mirror of the
host code's rules."""
import pytest
import torch
import torch.nn.functional as F

import _thin_ref as tr

MUTANTS = ("noflip", "pad_off", "last_col", "last_block", "bias_twice", "asum_s", "trunc", "bf16_acc")
PRECISION = ("trunc", "bf16_acc")       # must be seen by a real-valued case; the others by an exact one


def _bf(v, mut):
    if mut == "trunc":
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return v.to(torch.bfloat16)


def _canvas(s, He, We, p):
    """float [N][He][We] with [n][i][j] = s[n][i - p][j - p], zero outside"""
    N, Hs, Ws = s.shape
    big = s.new_zeros((N, p + max(Hs, He), p + max(Ws, We)), dtype=torch.float32)
    big[:, p:p + Hs, p:p + Ws] = s.float()
    return big[:, :He, :We]


def _taps(x, wk, K, Ho, Wo, b):
    """the mutant that keeps its accumulator in bf16: one rounding per tap. x [N][Cin][Ho + K - 1][Wo + K - 1], wk [Cout][Cin][K][K]"""
    acc = (b if b is not None else x.new_zeros(wk.shape[0])).bfloat16().float().reshape(1, -1, 1, 1)
    for ky in range(K):
        for kx in range(K):
            term = torch.einsum("nchw,oc->nohw", x[:, :, ky:ky + Ho, kx:kx + Wo], wk[:, :, ky, kx])
            acc = (acc + term).bfloat16().float()
    return acc


def emulate(c, mut=None):
    K, pad, KK = c.K, c.pad, c.K * c.K
    flip = 0 if mut == "noflip" else c.flip
    p = pad + 1 if mut == "pad_off" else pad
    o = c.ops
    if c.kind in ("expand", "squeeze"):
        w = (o["w"].flip(1) if flip else o["w"]).float()
        b = o["b"]
        if c.kind == "expand":
            x = o["s"].float()[:, None]
            wk = w.reshape(-1, 1, K, K)
        else:
            x = o["a"].float().permute(0, 3, 1, 2)
            wk = w.reshape(1, -1, K, K)
        Ho, Wo = x.shape[2] + 2 * pad - K + 1, x.shape[3] + 2 * pad - K + 1
        x = F.pad(x, (p, p, p, p))[:, :, :Ho + K - 1, :Wo + K - 1]
        y = _taps(x, wk, K, Ho, Wo, b) if mut == "bf16_acc" else F.conv2d(x, wk, b)
        if mut == "bias_twice" and b is not None:
            y = y + b.reshape(1, -1, 1, 1)
        y = torch.where(y > 0, y, y * torch.tensor(c.slope, dtype=torch.float32))
        y = _bf(y, mut)
        if mut == "last_col":
            y[..., Wo - 1] = 0
        return dict(out=y.permute(0, 2, 3, 1).contiguous() if c.kind == "expand" else y[:, 0].contiguous())
    a, s = o["a"].float().clone(), o["s"]
    N, Ha, Wa, C = a.shape
    if mut == "last_col":
        a[:, :, Wa - 1] = 0
    if mut == "last_block":
        rows = tr.WG_ROWS_WIDE if c.form == "wide" else tr.WG_ROWS
        a.view(N * Ha, Wa, C)[(c.blocks - 1) * rows:] = 0
    win = _canvas(s, Ha + K - 1, Wa + K - 1, p)
    if mut == "bf16_acc":
        g = a.new_zeros((C, K, K))
        for n in range(N):
            for y in range(Ha):       # one rounding per row of a
                g = (g + F.conv2d(win[None, n:n + 1, y:y + K], a[n:n + 1, y:y + 1].permute(3, 0, 1, 2))[0]).bfloat16().float()
    else:
        g = F.conv2d(win[None], a.permute(3, 0, 1, 2))[0]              # [C][K][K]: sum over n, y, x of a[n,y,x,c] * win[n,y+ky,x+kx]
    g = g.reshape(C, KK)
    asum = s.float().sum().expand(C).clone() if mut == "asum_s" else a.sum((0, 1, 2))
    return dict(g=(g.flip(1) if flip else g).contiguous(), asum=asum)


def _rejected(c, r, mut):
    return any(not v <= 1.0 for v in tr.check(c, r, emulate(c, mut)).values())


def test_every_case_runs_the_kernel_it_is_listed_under_and_covers_the_dispatch():
    forms = {(c.fam, c.form) for c in (tr.case(*k) for k in tr.ALL)}
    assert forms == {("expand", "expand"), ("squeeze_wide", "wide"), ("squeeze_lane", "lane"), ("wgrad_wide", "wide"), ("wgrad_lane", "lane")}
    assert sorted({tr.case("wgrad_wide", n, "exact").blocks for n in tr.WGRAD_WIDE_CASES}) == [1, 2, 3, 15, 16, 17, 32, 33, 48, 49]


def test_exact_cases_have_one_legal_result_and_the_emulation_gives_it():
    for key in tr.ALL:
        if key[2] != "exact":
            continue
        c, r = tr.case(*key), tr.ref_cpu(*key)       # ref_of asserts S < 2^20
        for name, _, bf16 in tr.outputs(c):
            ref = getattr(r, name)
            assert torch.equal(ref.float().double(), ref) and torch.equal(ref * 64, (ref * 64).round()), key      # 2^-4 products, slope 2^-2
        rat = tr.check(c, r, emulate(c))
        assert all(v == 0.0 for v in rat.values()), (key, rat)


def test_exact_cases_contain_rounding_ties_and_inexact_values():
    """the bf16 outputs of the exact cases must make the ONE rounding visible: values bf16 cannot hold, and exact ties"""
    ties = inexact = 0
    for key in tr.ALL:
        c = tr.case(*key)
        if key[2] != "exact" or c.kind == "wgrad":
            continue
        ref = tr.ref_cpu(*key).out.float()
        bits = ref.view(torch.int32) & 0xFFFF
        inexact += int((bits != 0).sum())
        ties += int((bits == 0x8000).sum())
    print(f"exact cases: {inexact} outputs need the rounding, {ties} of them are ties")
    assert inexact > 1000 and ties > 100


def test_emulated_kernels_are_within_every_bound():
    worst = {}
    for key in tr.ALL:
        if key[2] != "real":
            continue
        c, r = tr.case(*key), tr.ref_cpu(*key)
        rat = tr.check(c, r, emulate(c), worst)
        assert all(v <= 1.0 for v in rat.values()), (key, rat)
    for k in sorted(worst):
        print(f"RATIO emulation {k} {worst[k]:.4f}")
    assert len(worst) == 7          # out of expand, 2 x squeeze; g and asum of 2 x wgrad


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_rejected(mut):
    caught = [f"{k[0]}/{k[1]}/{k[2]}" for k in tr.ALL if _rejected(tr.case(*k), tr.ref_cpu(*k), mut)]
    print(mut, "rejected by", len(caught), "cases:", caught)
    want = "/real" if mut in PRECISION else "/exact"
    assert any(n.endswith(want) for n in caught), f"no {want[1:]} case notices the mutant {mut}"


def test_chain_lengths():
    assert tr.chain("expand", 7, 64) == 51 and tr.chain("squeeze", 4, 512) == 16 * 8 + 8 and tr.chain("squeeze", 3, 8) == 17
    # wide wgrad, C = 64: 8 pixel lanes (3 folds), Wa = 37 -> 10 quads -> 2 per thread = 8 pixels, 4 rows; 3 blocks
    assert tr.chain("wgrad", 7, 64, Wa=37, blocks=3) == 4 * 8 + 3 + 1 + 18
    # C = 512: one pixel lane, no fold, Wa = 9 -> 3 quads = 12 pixels; 33 blocks -> 2 laps of the reduction
    assert tr.chain("wgrad", 4, 512, Wa=9, blocks=33) == 4 * 12 + 0 + 2 + 18
    # lane-per-channel: 2 rows x 29 pixels rounded up to 3 x 14; 17 blocks
    assert tr.chain("wgrad", 7, 192, Wa=29, blocks=17) == 2 * 42 + 1 + 18


def test_supported_admits_only_what_the_native_side_accepts():
    from octa_autosegmentation_amd.models import thin_conv
    admitted = set()
    for K in (4, 7):
        for C in range(64, 1025, 64):
            for pad in range(K + 1):
                for conv in (torch.nn.Conv2d(1, C, K, 1, pad), torch.nn.Conv2d(C, 1, K, 1, pad)):
                    if not thin_conv.supported(conv):
                        continue
                    admitted.add((K, C))
                    # either layer runs all three entry points: forward, data gradient (padding K - 1 - pad) and weight gradient
                    assert tr.shape_ok(C, K, pad) and tr.shape_ok(C, K, K - 1 - pad), (K, C, pad)
                    assert tr.expand_ok(C, K) and tr.squeeze_form(C, K) is not None and tr.wgrad_form(C, K) is not None, (K, C, pad)
    # and the layers the networks have are admitted: generator stem / head (7 x 7, 64), discriminator stem / head (4 x 4, 64 / 512)
    assert {(7, 64), (4, 64), (4, 512)} <= admitted
    assert thin_conv.supported(torch.nn.Conv2d(1, 64, 7)) and thin_conv.supported(torch.nn.Conv2d(64, 1, 7))
    assert thin_conv.supported(torch.nn.Conv2d(1, 64, 4, 1, 1)) and thin_conv.supported(torch.nn.Conv2d(512, 1, 4, 1, 1))
    print("supported() admits", sorted(admitted))
    # the two shapes whose weights fit neither form's LDS table, and the C the lane-per-channel forms take
    assert tr.squeeze_form(512, 7) is None and tr.squeeze_form(1024, 4) is None
    assert [C for C in range(64, 1025, 64) if tr.squeeze_form(C, 4) == "lane"] == [192, 320, 384, 448, 576, 640, 704, 768, 832, 896, 960]
    assert tr.squeeze_form(320, 7) == "lane" and tr.squeeze_form(384, 7) is None
    assert tr.wgrad_form(1024, 7) == "lane" and tr.wgrad_form(512, 7) == "wide"
