"""Proves tests/_conv_ref.py without a GPU: an emulation of the arithmetic of csrc/conv.hip in torch on the CPU -- fp32 sums on the bf16
operands in the kernels' order (per 16-channel slice, then per tap, for the forward; per tile, then folded, for the weight gradient), one
rounding to bf16 -- reproduces every exact case bit for bit and stays inside the bound of every real-valued case that
tests/test_conv_exact_gpu.py runs; the float64 reference agrees with torch's own convolutions in float64; each of a list of wrong kernels
(mutants of the emulation) is rejected by the cases named beside it; and the mirror of the host code's dispatch reaches every
instantiation the entry points can launch, for 256 and for 304 compute units."""
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as cr

# mutant -> the cases that have to reject it
EXACT_MUTANTS = {
    "tap_transposed": [("fwd", "bn32_wo31_ho7"), ("fwd4", "bn32_pad1_9x34"), ("wgrad", "f32x32_4x31")],
    "tap_flip": [("fwd", "bn64_wo31_ho7"), ("s2t", "8x32"), ("wgrad", "f64x64_4x31")],
    "dil_parity": [("fwd", "bn32_dil2_wo34"), ("s2t", "9x33_n2")],
    "last_col": [("fwd", "bn32_wo33_ho9_n3"), ("wgrad", "f64x64_8x33"), ("wgrad", "f32x32_norm")],
    "c1_off": [("fwd", "bn32_c1_32of96"), ("fwd", "bn64_c1_96of128"), ("wgrad", "c1_32of64")],
    "cy1_ignored": [("fwd", "cy1_32of96"), ("fwd", "cy1_64of128")],
    "scatter_swapped": [("fwd", "bn32_scatter_01"), ("fwd", "bn64_scatter_10")],
    "scatter_all": [("fwd", "bn32_scatter_00"), ("fwd", "bn64_scatter_11")],
    "reflect_edge": [("fwd_pad", "reflect_2x2"), ("fwd_pad", "reflect_9x8"), ("wgrad_pad", "reflect_2x2_f32x32"), ("wgrad_pad", "reflect_9x33_f64x64")],
    "wgrad_mask_ignored": [("wgrad", "f32x32_mask"), ("wgrad", "f64x64_mask_set"), ("wgrad", "s2_f64x32_10x66_convt")],
    "add_overwrites": [("wgrad", "pb16_add"), ("wgrad", "pb88_add")],
    "set_adds": [("wgrad", "pb16_set"), ("wgrad", "pb88_set")],
    "s2_pairing": [("wgrad", "s2_f32x32_2x2"), ("wgrad", "s2_f64x32_10x66")],
    "res_before_rounding": [("fwd", "bn32_res_s1"), ("s2t", "res_9x33")],
    "stats_unrounded": [("fwd", "bn32_stats_large_values"), ("fwd", "bn64_stats_large_values")],
}
REAL_MUTANTS = {
    "trunc": [("fwd", "bn32_wo31_ho7"), ("fwd4", "bn64_pad1_9x34"), ("s2t", "8x32")],
    "bf16_acc": [("fwd", "bn32_dil2_wo34"), ("wgrad", "f32x32_9x32")],
    "norm_noround": [("fwd", "bn32_norm_one"), ("wgrad", "f32x32_norm")],
}


def _bf(v, mut):
    if mut == "trunc":
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return v.to(torch.bfloat16)


def _layer_input(c, mut):
    """x1 | x2 as fp32 values of the bf16 numbers the kernel multiplies: normalise-on-load in fp32, rounded to bf16"""
    p, o = c.p, c.ops
    parts = []
    for i, key in ((1, "x"), (2, "x2")):
        if o.get(key) is None:
            continue
        v = o[key].float()
        if o.get(f"sc{i}") is not None:
            z = v * o[f"sc{i}"][:, None, None, :] + o[f"sh{i}"][:, None, None, :]
            z = torch.where(z > 0, z, z * torch.tensor(p.slope, dtype=torch.float32))
            v = z if mut == "norm_noround" else _bf(z, mut).float()
        parts.append(v)
    if mut == "c1_off" and len(parts) == 2:          # the last slice below the split is read from the second tensor
        parts[0] = torch.cat((parts[0][..., :-16], parts[1][..., :16]), 3)
    X = torch.cat(parts, 3)
    if mut == "last_col" and p.W == 33:
        X[:, :, 32] = 0
    return X


def _padded(X, dil, pad, reflect, mut, extra=0):
    """[N][H][W][C] -> the virtual, padded image [N][H dil + 2 pad (+ extra)][..][C]"""
    N, H, W, C = X.shape
    if dil == 2:
        if mut == "dil_parity":
            Xv = X.repeat_interleave(2, 1).repeat_interleave(2, 2)
        else:
            Xv = X.new_zeros((N, 2 * H, 2 * W, C))
            Xv[:, ::2, ::2] = X
    else:
        Xv = X
    Xv = Xv.permute(0, 3, 1, 2)
    if reflect:
        Xv = F.pad(Xv, (pad, pad, pad, pad), mode="replicate" if mut == "reflect_edge" else "reflect")
        Xv = F.pad(Xv, (0, extra, 0, extra))
    else:
        Xv = F.pad(Xv, (pad, pad + extra, pad, pad + extra))
    return Xv.permute(0, 2, 3, 1)


def _tap_of(t, K, mut):
    if mut == "tap_transposed":
        return K * (t % K) + t // K
    return K * K - 1 - t if mut == "tap_flip" else t


def _emulate_stats(c, v):
    """v [N][Ho][Wo][C] fp32 -> the statistics buffer, tile by tile"""
    p = c.p
    nslot = p.stats if isinstance(p.stats, int) else 0
    N, Ho, Wo, C = v.shape
    th = c.d.THT if nslot else 8
    ty, tx = (Ho + th - 1) // th, (Wo + cr.TW - 1) // cr.TW
    tiles = torch.zeros((N, ty * tx, C, 2), dtype=torch.float32)
    slots = torch.zeros((max(nslot, 1), N, C, 2), dtype=torch.float64)
    for t in range(ty * tx):
        blk = v[:, (t // tx) * th:(t // tx + 1) * th, (t % tx) * cr.TW:(t % tx + 1) * cr.TW]
        tiles[:, t, :, 0], tiles[:, t, :, 1] = blk.sum((1, 2)), (blk * blk).sum((1, 2))
        slots[t % max(nslot, 1)] += tiles[:, t].double()
    return slots if nslot else tiles


def emulate(c, mut=None):
    p, o = c.p, c.ops
    K, KK, st = p.K, p.K * p.K, p.stride
    Ho, Wo = cr.out_extent(p)
    X = _layer_input(c, mut)
    if c.fam in cr.FORWARD:
        Xp = _padded(X, p.dil, p.pad, p.reflect, mut)
        w = o["w"].float()
        acc = torch.zeros((p.N, Ho, Wo, p.Cout), dtype=torch.float32)
        for c0 in range(0, p.Cin, 16):
            for t in range(KK):
                if (p.mask >> t) & 1:
                    r, s = t // K, t % K
                    g = Xp[:, r:r + (Ho - 1) * st + 1:st, s:s + (Wo - 1) * st + 1:st, c0:c0 + 16]
                    acc += torch.einsum("nyxc,oc->nyxo", g, w[_tap_of(t, K, mut)][:, c0:c0 + 16])
            if mut == "bf16_acc":
                acc = acc.bfloat16().float()
        y = _bf(acc, mut)
        if p.res:
            y = _bf(acc + o["res"].float(), mut) if mut == "res_before_rounding" else _bf(y.float() + o["res"].float(), mut)
        got = dict(y=y, y2=None, stats=None)
        if p.stats is not None:
            got["stats"] = _emulate_stats(c, acc if mut == "stats_unrounded" else y.float())
        if p.scatter:
            osc, a, b = p.scatter
            if mut == "scatter_swapped":
                a, b = b, a
            full = torch.full((p.N, Ho * osc, Wo * osc, p.Cout), cr.SENT_BITS, dtype=torch.int16).view(torch.bfloat16)
            if mut == "scatter_all":
                full = y.repeat_interleave(osc, 1).repeat_interleave(osc, 2)
            else:
                full[:, a::osc, b::osc] = y
            got["y"] = full
        elif p.CY1:
            got["y"], got["y2"] = y[..., :p.CY1].contiguous(), y[..., (0 if mut == "cy1_ignored" else p.CY1):][..., :p.Cout - p.CY1].contiguous()
        return got
    pad = 0 if (mut == "s2_pairing" and st == 2) else p.pad
    Xp = _padded(X, 1, pad, p.reflect, mut, extra=2)
    dy = o["dy"].float()
    th = c.d.TH_
    g = torch.zeros((KK, p.Cout, p.Cin), dtype=torch.float32)
    for n in range(p.N):
        for y0 in range(0, Ho, th):                  # one tile row of the image at a time, folded in fp32
            y1 = min(Ho, y0 + th)
            part = torch.zeros_like(g)
            for t in range(KK):
                if (p.mask >> t) & 1 or mut == "wgrad_mask_ignored":
                    r, s = t // K, t % K
                    gx = Xp[n, y0 * st + r:(y1 - 1) * st + r + 1:st, s:s + (Wo - 1) * st + 1:st]
                    part[_tap_of(t, K, mut)] = torch.einsum("yxo,yxc->oc", dy[n, y0:y1], gx)
            g = g + part
            if mut == "bf16_acc":
                g = g.bfloat16().float()
    if p.mode != cr.TAP_MAJOR:
        g = g.view(3, 3, p.Cout, p.Cin).permute(2, 3, 0, 1).contiguous()
        if p.mode == cr.PARAM_ADD and mut != "add_overwrites":
            g = g + o["base"]
        if p.mode == cr.PARAM_SET and mut == "set_adds":
            g = g + 1.0                              # whatever the buffer held
    return dict(dw=g)


def _rejected(key, mut):
    c, r = cr.case(*key), cr.ref_cpu(*key)
    return any(not v <= 1.0 for v in cr.check(c, r, emulate(c, mut)).values())


def test_every_case_runs_the_kernel_it_is_listed_under_and_the_list_covers_the_dispatch():
    for cus in cr.NUM_CUS:
        insts, pbs, folds = set(), set(), set()
        for key in cr.ALL:
            c = cr.case(*key, cus)                   # asserts instantiation, fold path, per_block
            insts.add(c.d.inst)
            if c.fam not in cr.FORWARD:
                pbs.add(c.d.per_block)
                folds.add(c.d.fold)
                if c.d.fold_inst:
                    insts.add(c.d.fold_inst)
        want = cr.fwd_instantiations() | cr.wgrad_instantiations()
        assert insts == want, (cus, sorted(want - insts), sorted(insts - want))
        assert len(cr.fwd_instantiations()) == 25
        assert len(cr.wgrad_instantiations()) == 40      # 32 gradient kernels + 8 folding kernels
        assert {1, 15, 16, 64} <= pbs and max(pbs) >= 65 and folds == {"atomics", "workspace", "acc", "slices"}, (cus, sorted(pbs), folds)


def test_the_mirror_refuses_every_call_of_the_refusal_list():
    for name, (p, extra) in cr.REFUSALS.items():
        why = (cr.fwd_refusal if p.kind in cr.FORWARD else cr.wgrad_refusal)(p, **extra)
        assert why, name
    for fam in cr.FAMILIES:                       # and none of the cases
        for name, (_, p) in cr.FAMILIES[fam].items():
            assert not (cr.fwd_refusal if fam in cr.FORWARD else cr.wgrad_refusal)(p), (fam, name)


def test_exact_cases_have_one_legal_result_and_the_emulation_gives_it():
    ties = inexact = 0
    for key in cr.ALL:
        if key[2] != "exact":
            continue
        c, r = cr.case(*key), cr.ref_cpu(*key)       # ref_of asserts S, the normalised inputs and the sum of squares
        ref = r.acc if c.fam in cr.FORWARD else r.g
        assert torch.equal(ref.float().double(), ref) and torch.equal(ref * 128, (ref * 128).round()), key
        if c.fam in cr.FORWARD:
            bits = ref.float().view(torch.int32) & 0xFFFF
            inexact += int((bits != 0).sum())
            ties += int((bits == 0x8000).sum())
        rat = cr.check(c, r, emulate(c))
        assert all(v == 0.0 for v in rat.values()), (key, rat)
    print(f"exact cases: {inexact} outputs need the rounding, {ties} of them are ties")
    assert inexact > 10000 and ties > 1000       # the ONE rounding is visible: values bf16 cannot hold, and exact ties


def test_emulated_kernels_are_within_every_bound():
    worst = {}
    for key in cr.ALL:
        if key[2] != "real":
            continue
        c, r = cr.case(*key), cr.ref_cpu(*key)
        assert c.p.Cin <= 64, key
        rat = cr.check(c, r, emulate(c), worst)
        assert all(v <= 1.0 for v in rat.values()), (key, rat, c.D)
    for k in sorted(worst):
        print(f"RATIO emulation {k} {worst[k]:.4f}")
    assert {k.split(".")[0] for k in worst} == set(cr.FAMILIES)


@pytest.mark.parametrize("mut", list(EXACT_MUTANTS))
def test_indexing_mutant_is_rejected_by_its_exact_cases(mut):
    for fam, name in EXACT_MUTANTS[mut]:
        assert _rejected((fam, name, "exact"), mut), f"{fam}/{name}/exact does not notice the mutant {mut}"


@pytest.mark.parametrize("mut", list(REAL_MUTANTS))
def test_precision_mutant_is_rejected_by_its_real_valued_cases(mut):
    for fam, name in REAL_MUTANTS[mut]:
        assert _rejected((fam, name, "real"), mut), f"{fam}/{name}/real does not notice the mutant {mut} at r = {cr.R_MFMA}"


def test_chain_lengths():
    c = cr.case("fwd", "bn32_dil2_wo34", "real")
    assert c.D == 9 * 4 * cr.R_MFMA + 1
    assert cr.case("fwd", "bn32_mask_convt", "real").D == 4 * 2 * cr.R_MFMA + 1 and cr.case("fwd4", "bn32_pad1_2x2", "real").D == 16 * 2 * cr.R_MFMA + 1
    # 64 x 64 blocks: one wave per pair takes the 8 rows of a tile: 16 instructions per tap; 2 x 2 tiles, one per workgroup: 4 atomic arrivals
    assert cr.case("wgrad", "f64x64_8x33", "real").D == 16 * cr.R_MFMA + 0 + 4
    # 32 x 32 blocks: four waves share the pair (2 rows each, 3 folds); 88 workgroups into the parameter layout in 2 slices of 44
    assert cr.case("wgrad", "pb88_add", "real").D == 4 * cr.R_MFMA + 3 + (11 + 3 + 2)
    assert cr.case("wgrad", "pb16_tap", "real").D == 4 * cr.R_MFMA + 3 + (4 + 3) and cr.case("wgrad", "pb15_tap", "real").D == 4 * cr.R_MFMA + 3 + 15
    # register-staged, 64 x 32: two waves per pair, 2 rows each: 4 instructions per tap and tile; 2 x 3 x 2 tiles, every wave adds its own
    assert cr.case("wgrad", "f64x32_norm", "real").D == 4 * cr.R_MFMA + 12 * 2


# ---- the reference against torch's own convolutions in float64 (guards the hand-written indexing) -----------------------------------------

def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _param(w, K):
    """nominal [KK][Cout][Cin] -> [Cout][Cin][K][K]"""
    return w.double().view(K, K, w.shape[1], w.shape[2]).permute(2, 3, 0, 1)


@pytest.mark.parametrize("fam,name", [("fwd", "bn32_wo33_ho9_n3"), ("fwd", "bn32_s2_odd"), ("fwd", "bn64_s2_even"), ("fwd", "bn32_dil2_wo34"), ("fwd", "bn32_c1_32of96"),
                                      ("fwd_pad", "pad0_10x35"), ("fwd_pad", "pad2_7x31"), ("fwd_pad", "reflect_9x8"), ("fwd_pad", "reflect_2x2"),
                                      ("s2t", "9x33_n2"), ("fwd4", "bn32_pad1_9x34"), ("fwd4", "bn64_pad3_1x1")])
def test_forward_reference_agrees_with_torch(fam, name):
    c, r = cr.case(fam, name, "exact"), cr.ref_cpu(fam, name, "exact")
    p, o = c.p, c.ops
    x = _nchw(torch.cat([t for t in (o["x"], o.get("x2")) if t is not None], 3))
    wp = _param(o["w"], p.K)
    if p.dil == 2:          # the zero insertion is a transposed convolution with the flipped kernel
        want = F.conv_transpose2d(x, wp.flip(2, 3).permute(1, 0, 2, 3), stride=2, padding=1, output_padding=1)
    elif p.reflect:
        want = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wp)
    else:
        want = F.conv2d(x, wp, stride=p.stride, padding=p.pad)
    assert torch.equal(want.permute(0, 2, 3, 1), r.acc)          # exact operands: every float64 sum is exact


@pytest.mark.parametrize("fam,name", [("wgrad", "f32x32_8x33"), ("wgrad", "f64x32_4x31"), ("wgrad", "s2_f32x32_10x66"), ("wgrad", "s2_f64x32_2x2"), ("wgrad", "c1_32of64"),
                                      ("wgrad", "pb15_set"), ("wgrad_pad", "pad0_3x3"), ("wgrad_pad", "pad2_1x1"), ("wgrad_pad", "reflect_9x33_f32x32"),
                                      ("wgrad_pad", "reflect_2x2_f64x64"), ("wgrad4", "c32_5x34"), ("wgrad4", "c64_2x2")])
def test_weight_gradient_reference_agrees_with_autograd(fam, name):
    c, r = cr.case(fam, name, "exact"), cr.ref_cpu(fam, name, "exact")
    p, o = c.p, c.ops
    x = _nchw(torch.cat([t for t in (o["x"], o.get("x2")) if t is not None], 3))
    wp = torch.zeros((p.Cout, p.Cin, p.K, p.K), dtype=torch.float64, requires_grad=True)
    if p.reflect:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wp)
    else:
        y = F.conv2d(x, wp, stride=p.stride, padding=p.pad)
    y.backward(_nchw(o["dy"]))
    want = wp.grad if p.mode else wp.grad.permute(2, 3, 0, 1).reshape(p.K * p.K, p.Cout, p.Cin)
    assert torch.equal(want, r.g)


def test_masked_reference_is_the_convolution_with_the_cleared_taps_zeroed():
    c, r = cr.case("fwd", "bn32_mask_asym", "exact"), cr.ref_cpu("fwd", "bn32_mask_asym", "exact")
    w = c.ops["w"].clone()
    for t in range(9):
        if not (c.p.mask >> t) & 1:
            w[t] = 0
    assert torch.equal(F.conv2d(_nchw(c.ops["x"]), _param(w, 3), padding=1).permute(0, 2, 3, 1), r.acc)
    c, r = cr.case("wgrad", "s2_f32x32_10x66_convt", "exact"), cr.ref_cpu("wgrad", "s2_f32x32_10x66_convt", "exact")
    assert all(bool((r.g[t] == 0).all()) == (not (0x1b0 >> t) & 1) for t in range(9))
