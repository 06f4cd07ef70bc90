"""Proves tests/_conv_f32_ref.py without a GPU: (a) the float64 references agree with torch's own convolutions and with float64 autograd;
(b) an emulation of the arithmetic of csrc/conv_f32.hip in torch on the CPU -- fp32 accumulators, one rounding per product, in the kernels'
order (forward: per slice of KC channels, per channel pair, per tap, two channels per instruction; weight gradient: per tile, per wave, pixel
by pixel, then the four waves folded in order, then the chunks in order; bias gradient: per thread, tree, fold) -- reproduces every exact
case bit for bit and stays inside the bound of every real-valued case that tests/test_conv_f32_exact_gpu.py runs; (c) each of a list of
wrong kernels (mutants of the emulation) is rejected by the cases named beside it; (d) the mirror of the host code reaches all 15 forward and
all 4 weight-gradient instantiations, for 256 and for 304 compute units; (e) no case is skipped and no element left out of a comparison."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import _conv_f32_ref as cr

# mutant -> the cases that have to reject it
EXACT_MUTANTS = {
    "taps_transposed": [("fwd", "k3s1_wo31_ho7"), ("fwd", "k4s1_wo32_ho8"), ("fwd", "k7s1_wo33_ho9_n3"), ("dgrad", "t22_24_20"), ("wgrad", "c31_8x32")],
    "dgrad_no_flip": [("dgrad", "c31_wo31"), ("dgrad", "c31_wo33_n3")],
    "dgrad_pad_off": [("dgrad", "c31_wo32"), ("dgrad", "c31_1_1")],
    "parity_R_swapped": [("dgrad", "c32_odd_n3"), ("dgrad", "c32_even"), ("dgrad", "c32_odd_even")],
    "hp_wp_floor": [("dgrad", "c32_odd_n3"), ("dgrad", "c32_1x5"), ("dgrad", "c32_5x1"), ("dgrad", "c32_1x1")],
    "scatter_swapped": [("fwd", "k1s1_scatter_01"), ("fwd", "k1s1_scatter_10"), ("fwd", "k3s2_scatter_10"), ("dgrad", "c32_even")],
    "tr_col_parity": [("tr", "24_20_n2"), ("tr", "9_33"), ("tr", "1_1")],
    "kg_dropped": [("fwd", "k3s1_wo32_ho8"), ("fwd", "k7s1_cout72_n3"), ("tr", "8_72"), ("dgrad", "t22_40_5_n3")],
    "cout_w_ignored": [("fwd", "k3s1_coutw"), ("fwd", "k1s1_scatter_11"), ("dgrad", "c32_even")],
    "last_col": [("fwd", "k3s1_wo33_ho9_n3"), ("fwd", "k7s1_pad0"), ("tr", "24_20_n2"), ("dgrad", "c32_even"), ("wgrad", "c31_9x33_n3"), ("wgrad", "t22_ho3")],
    "ragged_dropped": [("wgrad", "c11_rounds"), ("wgrad", "c31_rounds"), ("wgrad", "c32_rounds"), ("wgrad", "t22_rounds")],
    "wave_left_out": [("wgrad", "c31_8x32"), ("wgrad", "c32_ho2_n3"), ("wgrad", "c11_7x31")],
    "tile_image": [("wgrad", "c31_9x33_n3"), ("wgrad", "c11_rounds"), ("wgrad", "t22_ho2_n3")],
    "bias_last_chunk": [("wgrad", "c31_9x33_n3"), ("wgrad", "c11_bias_35")],
    "bias_twice": [("fwd", "k3s1_wo31_ho7"), ("fwd", "k1s1_scatter_01")],
}
REAL_MUTANTS = {
    "tf32": [("fwd", "k3s1_wo33_ho9_n3"), ("fwd", "k7s1_wo31_ho7"), ("tr", "24_20_n2"), ("dgrad", "c31_wo32"), ("wgrad", "c31_8x32"), ("wgrad", "c32_ho1")],
    "bf16": [("fwd", "k1s1_wo32_ho8"), ("fwd", "k4s1_wo33_ho9_n3"), ("tr", "9_33"), ("dgrad", "c32_even"), ("wgrad", "c11_9x33_n3"), ("wgrad", "t22_ho2_n3")],
}


def _operand(v, mut):
    """an operand as a kernel that rounded it to 10 (xf32 / tf32) or 7 (bf16) mantissa bits would multiply it"""
    if mut == "tf32":
        b = v.contiguous().view(torch.int32)
        return ((b + 0xFFF + ((b >> 13) & 1)) & ~0x1FFF).view(torch.float32)
    return v.bfloat16().float() if mut == "bf16" else v


def _fma(acc, a, b):
    """fl(acc + a * b): the product is exact in float64"""
    return (acc.double() + a.double() * b.double()).float()


def _emulate_product(x, wflat, L, bias, mut):
    """one launch of conv_f32_kernel -> [N][Cout][Ho][Wo] fp32"""
    K, KK, k = L.K, L.K * L.K, cr.kc(L.K, L.S)
    w = cr.weights_of(wflat, L)
    G = [cr.gather(x, L.Ho, L.Wo, L.S, L.pad, t // K, t % K) for t in range(KK)]
    acc = torch.zeros((L.N, L.Cout, L.Ho, L.Wo), dtype=torch.float32)
    for c0 in range(0, L.Cin, k):
        for cp in range(0, k, 2):
            for t in range(KK):
                tw = K * (t % K) + t // K if mut == "taps_transposed" else (KK - 1 - t if mut == "dgrad_no_flip" else t)
                for ci in (c0 + cp, c0 + cp + 1):                 # the two products of one instruction
                    if ci < L.Cin:
                        acc = _fma(acc, G[t][:, ci, None], w[ci, tw][None, :, None, None])
    if bias is not None:
        acc = acc + bias[None, :, None, None]
        if mut == "bias_twice":
            acc = acc + bias[None, :, None, None]
    return acc


def _kg_dropped(v):
    """the register-to-channel map without the 4 * kg term: both half-waves store to channels (k & 3) + 8 (k >> 2) of the M-block (the second
    half-wave's value stays), channels with bit 2 set are never stored"""
    co = torch.arange(v.shape[1])
    out = v.clone()
    lo = (co & 4) == 0
    src = co[lo] + 4
    ok = src < v.shape[1]
    out[:, co[lo][ok]] = v[:, src[ok]]
    return out, lo


def _emulate_launches(c, mut):
    p = c.p
    o = {k: (_operand(v, mut) if k != "bias" else v) for k, v in c.ops.items()}
    src = o["dy"] if c.fam == "dgrad" else o["x"]
    wflat = cr.packed_weights(p, o)
    if mut == "parity_R_swapped" and p.stride == 2:
        wd = wflat.view(4, p.Cout, 2, 2, p.Cin).clone()
        for a in (0, 1):
            for b in (0, 1):
                if a:
                    wd[2 * a + b] = wd[2 * a + b].flip(1)
                if b:
                    wd[2 * a + b] = wd[2 * a + b].flip(2)
        wflat = wd.reshape(-1)
    L0 = c.Ls[0]
    y = torch.full((L0.N, L0.Cout, L0.Hy, L0.Wy), cr.SENT_BITS, dtype=torch.int32).view(torch.float32)
    for L in c.Ls:
        L = SimpleNamespace(**vars(L))
        if mut == "dgrad_pad_off" and c.fam == "dgrad" and L.K == 3:
            L.pad -= 1
        if mut == "hp_wp_floor" and L.osc == 2 and c.fam == "dgrad":
            L.Ho, L.Wo = (p.H - L.ooy) // 2, (p.W - L.oox) // 2
            if L.Ho <= 0 or L.Wo <= 0:
                continue
        if mut == "scatter_swapped":
            L.ooy, L.oox = L.oox, L.ooy
        if mut == "cout_w_ignored":
            L.cout_w = L.Cout
        parts = []
        if L.TR:
            for a in (0, 1):
                for b in (0, 1):
                    Lt = SimpleNamespace(**dict(vars(L), w_off=(2 * a + b) * L.Cout))
                    parts.append((a, 1 - b if mut == "tr_col_parity" else b, _emulate_product(src, wflat, Lt, None, mut)))
        else:
            parts.append((L.ooy, L.oox, _emulate_product(src, wflat, L, o.get("bias") if L.bias else None, mut)))
        for a, b, v in parts:
            keep = torch.ones(v.shape[1], dtype=torch.bool)
            if mut == "kg_dropped":
                v, keep = _kg_dropped(v)
            wo = L.Wo - 1 if (mut == "last_col" and L.Wo == 33) else L.Wo
            dst = y[:, :, a::L.osc, b::L.osc]
            dst[:, keep, :L.Ho, :wo] = v[:, keep, :, :wo]
    return dict(y=y)


def _emulate_wgrad(c, mut):
    p, d = c.p, c.d
    o = {k: _operand(v, mut) for k, v in c.ops.items()}
    x, dy = (o["dy"], o["x"]) if p.transposed else (o["x"], o["dy"])
    K, KK, S, th = p.K, p.K * p.K, p.stride, d.TH
    N, Cin = x.shape[0], x.shape[1]
    Cout, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    Hp, Wp = -(-Ho // th) * th, d.tiles_x * cr.TW
    dyp = F.pad(dy, (0, Wp - Wo, 0, Hp - Ho))
    if mut == "last_col" and Wo == 33:
        dyp[..., 32] = 0
    gx = torch.stack([F.pad(cr.gather(x, Ho, Wo, S, p.pad, t // K, t % K), (0, Wp - Wo, 0, Hp - Ho)) for t in range(KK)])     # [KK][N][Cin][Hp][Wp]
    npix, ppw2 = th * cr.TW, th * cr.TW // 4                   # pixels of a tile; pixels of a wave (PPW pairs): pixel rr * 32 + p belongs to wave (pixel / 2) / PPW
    total = d.total_tiles
    if mut == "ragged_dropped":
        total = (d.total_tiles // d.nchunks) * d.nchunks
    dw = torch.zeros((Cout, Cin, KK), dtype=torch.float32)
    for chunk in range(d.nchunks):
        acc = torch.zeros((4, Cout, Cin, KK), dtype=torch.float32)
        for t in range(chunk, total, d.nchunks):
            n, rem = (0 if mut == "tile_image" else t // d.tiles_per_img), t % d.tiles_per_img
            ty0, tx0 = (rem // d.tiles_x) * th, (rem % d.tiles_x) * cr.TW
            D = dyp[n, :, ty0:ty0 + th, tx0:tx0 + cr.TW].reshape(Cout, 4, ppw2)
            X = gx[:, n, :, ty0:ty0 + th, tx0:tx0 + cr.TW].reshape(KK, Cin, 4, ppw2)
            if c.var == "exact":                               # every partial sum is an fp32 number: the order inside a wave's tile is immaterial
                acc = (acc.double() + torch.einsum("owp,tcwp->woct", D.double(), X.double())).float()
            else:
                for j in range(ppw2):                          # pixel by pixel (two per instruction), the four waves side by side
                    acc = _fma(acc, D[:, :, j].t()[:, :, None, None], X[:, :, :, j].permute(2, 1, 0)[:, None])
        v = acc[0]
        for w in (1, 2, 3):
            if not (mut == "wave_left_out" and w == 2):
                v = v + acc[w]
        dw = dw + v
    dw = dw.view(Cout, Cin, K, K)
    if mut == "taps_transposed":
        dw = dw.transpose(2, 3).contiguous()
    # the bias gradient: DB_CHUNKS contiguous ranges of a channel's N * Ho * Wo values
    seq = dy.permute(1, 0, 2, 3).reshape(Cout, -1)
    tot = seq.shape[1]
    per = (tot + cr.DB_CHUNKS - 1) // cr.DB_CHUNKS
    assert per == d.per
    last = (tot - 1) // per
    db = torch.zeros((Cout,), dtype=torch.float32)
    for chunk in range(cr.DB_CHUNKS):
        seg = seq[:, chunk * per:min(chunk * per + per, tot)]
        if mut == "bias_last_chunk" and chunk == last:
            seg = seg[:, :0]
        steps = -(-seg.shape[1] // 256) if seg.shape[1] else 0
        seg = F.pad(seg, (0, steps * 256 - seg.shape[1])).view(Cout, steps, 256)
        s = torch.zeros((Cout, 256), dtype=torch.float32)
        for j in range(steps):
            s = s + seg[:, j]
        w = 128
        while w:
            s = s[:, :w] + s[:, w:2 * w]
            w //= 2
        db = db + s[:, 0]
    return dict(dw=dw, db=db)


def emulate(c, mut=None):
    return _emulate_wgrad(c, mut) if c.fam == "wgrad" else _emulate_launches(c, mut)


def _rejected(key, mut):
    c, r = cr.case(*key), cr.ref_cpu(*key)
    return any(not v <= 1.0 for v in cr.check(c, r, emulate(c, mut)).values())


# ---- (d) the case list against the dispatch -------------------------------------------------------------------------------------------------

def _instantiations(cus):
    insts, changed = set(), []
    for fam, name, var in cr.ALL:
        if var != "exact":
            continue
        listed, p = cr.FAMILIES[fam][name]
        got = [cr.wgrad_dispatch(p).inst] if fam == "wgrad" else [L.inst for L in cr.launches(p, cus)]
        insts |= set(got)
        if got != listed:
            changed.append((fam, name))
    return insts, changed


def test_the_case_list_reaches_every_instantiation():
    want = cr.fwd_instantiations() | cr.wgrad_instantiations()
    assert len(cr.fwd_instantiations()) == 15 and len(cr.wgrad_instantiations()) == 4
    for key in cr.ALL:
        cr.case(*key)                                # asserts, for 256 compute units, the instantiations each case is listed under
    insts, changed = _instantiations(256)
    assert insts == want and not changed, (sorted(want - insts), changed)
    # 304 compute units (MI300X): balance() only matters at stride 1 with Cout > 32. No case of the list changes its kernel: the small
    # stride-1 cases have so few workgroups that both widths fill a fraction of one wave of workgroups (ratio 1/2 or 2/3: narrow), the wide
    # ones have 160 tiles, inside (128, 256] and (152, 304].
    insts, changed = _instantiations(304)
    assert insts == want and not changed, (sorted(want - insts), changed)


def test_the_balance_rule():
    # 33..64 output channels: wide exactly when the tiles of the batch fill more than half of the compute units' first round
    for cus, lo, hi in ((256, 128, 256), (304, 152, 304)):
        for tiles in (1, lo, lo + 1, hi, hi + 1, 2 * hi):
            wide = cr.wide(1, 64, 1, 8 * tiles, 32, cus)
            assert wide == (lo < tiles <= hi or tiles == 2 * hi), (cus, tiles)
    assert cr.wide(2, 40, 1, 40, 512, 256) and cr.wide(2, 64, 1, 40, 512, 304)
    assert cr.wide(1, 33, 2, 1, 1, 256) and not cr.wide(1, 32, 2, 100, 100, 256)
    # the layer cases the existing tests run at stride 1 stay narrow: Conv2d(128, 256) at 40 x 40, ConvTranspose2d(512, 256, 1, 1) at 24 x 24
    assert not cr.wide(1, 256, 1, 40, 40, 256) and not cr.wide(1, 256, 1, 24, 24, 256)


def test_the_weight_gradient_plan():
    d = cr.case("wgrad", "c11_rounds", "exact").d
    assert (d.tiles_per_img, d.total_tiles, d.ci_blocks, d.co_blocks, d.nchunks, d.rounds, d.ragged) == (6, 18, 8, 8, 16, 2, True)
    assert d.bytes == (16 * 64 * 1024 + 256 * 64) * 4 and d.D == 2 * 32 * 2 + 3 + 16
    for name in ("c31_rounds", "c32_rounds", "t22_rounds"):
        d = cr.case("wgrad", name, "exact").d
        assert (d.total_tiles, d.nchunks, d.rounds, d.ragged) == (66, 64, 2, True), name
        assert 64 // d.tiles_per_img != 0                    # tiles t and t + 64 of a workgroup lie in different images
    d = cr.case("wgrad", "c32_ho3", "real").d
    assert d.TH == 2 and d.total_tiles == 4 and d.D == 1 * 8 * 2 + 3 + 4
    d = cr.case("wgrad", "c31_9x33_n3", "real").d
    assert d.per == 14 and 297 % 14 != 0 and d.D_bias == 1 + 8 + 64 and d.D == 64 + 3 + 12
    assert cr.case("wgrad", "c11_bias_35", "real").d.per == 1


def test_chain_lengths():
    L = cr.case("fwd", "k3s1_wo33_ho9_n3", "real").Ls[0]
    assert L.Cin == 9 and L.D == 2 * 8 * 9 + 1
    assert cr.case("fwd", "k7s1_wo31_ho7", "real").Ls[0].D == 2 * 49 + 1 and cr.case("fwd", "k4s1_wo33_ho9_n3", "real").Ls[0].D == 2 * 4 * 16 + 1
    assert cr.case("fwd", "k3s2_wo31_ho7", "real").Ls[0].D == 4 * 9 + 1 and cr.case("fwd", "k1s1_cout64_nobias", "real").Ls[0].D == 8
    assert [L.D for L in cr.case("dgrad", "c32_even", "real").Ls] == [16, 64, 64, 64]          # the layer's Cout = 9: two slices of 8; 1 / 4 taps
    assert cr.case("tr", "24_20_n2", "real").Ls[0].D == 24


def test_the_mirror_refuses_every_call_of_the_refusal_list():
    for name, p in cr.REFUSALS.items():
        assert cr.refusal(p), name
    for fam in cr.FAMILIES:
        for name, (_, p) in cr.FAMILIES[fam].items():
            assert not cr.refusal(p), (fam, name)
    kinds = {(p.kind, cr.refusal(p)) for p in cr.REFUSALS.values()}
    assert {("fwd", "bad output scatter"), ("fwd", "reads beyond the padded input"), ("fwd", "is not instantiated"), ("dgrad", "is not covered"),
            ("dgrad", "the layer gives"), ("wgrad", "bad arguments"), ("wgrad", "needed"), ("tr", "the output must be 8-byte aligned")} <= kinds


def test_the_workspace_query_refuses_only_nonpositive_arguments():
    ok = dict(N=1, Cin=8, H=8, W=8, Cout=32, K=3, stride=1, pad=1, Ho=8, Wo=8)
    assert cr.workspace_refusal(**ok) is None and cr.workspace_refusal(**dict(ok, K=5, stride=3)) is None
    for k in ok:
        assert cr.workspace_refusal(**dict(ok, **{k: -1})) == "bad arguments", k
        assert (cr.workspace_refusal(**dict(ok, **{k: 0})) is None) == (k == "pad"), k


# ---- (b) the emulation ------------------------------------------------------------------------------------------------------------------------

def test_exact_cases_have_one_legal_result_and_the_emulation_gives_it():
    n = 0
    for key in cr.ALL:
        if key[2] != "exact":
            continue
        c, r = cr.case(*key), cr.ref_cpu(*key)       # ref_of asserts S < 2^20
        for ref in ((r.g, r.db) if c.fam == "wgrad" else (r.ref,)):
            assert torch.equal(ref.float().double(), ref) and torch.equal(ref * 16, (ref * 16).round()), key
        rat = cr.check(c, r, emulate(c))
        assert all(v == 0.0 for v in rat.values()), (key, rat)
        n += 1
    assert n == sum(len(v) for v in cr.FAMILIES.values())          # (e) every case has its exact variant and none is skipped


def test_emulated_kernels_are_within_every_bound():
    worst = {}
    for key in cr.ALL:
        if key[2] != "real":
            continue
        c, r = cr.case(*key), cr.ref_cpu(*key)
        assert c.fam == "wgrad" or max(L.Cin * L.K * L.K for L in c.Ls) <= 147, key            # terms per output: the bound stays sharp
        rat = cr.check(c, r, emulate(c), worst)
        assert all(v <= 1.0 for v in rat.values()), (key, rat)
    for k in sorted(worst):
        print(f"RATIO emulation {k} {worst[k]:.4f}")
    assert set(worst) == {"fwd.y", "fwd.untouched", "tr.y", "tr.untouched", "dgrad.y", "dgrad.untouched", "wgrad.dw", "wgrad.db"}


def test_no_element_is_left_out_of_a_comparison():
    """(e) a single wrong element anywhere -- first, last, or an unwritten one of a scattered launch -- fails the check of either family"""
    for key in (("fwd", "k1s1_scatter_10", "exact"), ("fwd", "k1s1_scatter_10", "real"), ("dgrad", "c32_odd_n3", "real"), ("tr", "9_33", "real")):
        c, r = cr.case(*key), cr.ref_cpu(*key)
        good = emulate(c)["y"]
        assert all(v <= 1.0 for v in cr.check(c, r, dict(y=good)).values())
        for idx in ((0, 0, 0, 0), (-1, -1, -1, -1), (0, 0, 0, 1), (0, 0, 1, 0), (-1, -1, -1, -2)):
            bad = good.clone()
            bad[idx] = bad[idx] * (1 + 2.0 ** -12) + 1.0
            assert any(not v <= 1.0 for v in cr.check(c, r, dict(y=bad)).values()), (key, idx)
    for key in (("wgrad", "c31_9x33_n3", "exact"), ("wgrad", "c31_9x33_n3", "real")):
        c, r = cr.case(*key), cr.ref_cpu(*key)
        good = emulate(c)
        for k in ("dw", "db"):
            for flat in (0, -1):
                bad = {q: v.clone() for q, v in good.items()}
                bad[k].view(-1)[flat] += 1.0
                assert any(not v <= 1.0 for v in cr.check(c, r, bad).values()), (key, k, flat)


# ---- (c) the mutants --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mut", list(EXACT_MUTANTS))
def test_indexing_mutant_is_rejected_by_its_exact_cases(mut):
    for fam, name in EXACT_MUTANTS[mut]:
        assert _rejected((fam, name, "exact"), mut), f"{fam}/{name}/exact does not notice the mutant {mut}"


@pytest.mark.parametrize("mut", list(REAL_MUTANTS))
def test_precision_mutant_is_rejected_by_its_real_valued_cases(mut):
    for fam, name in REAL_MUTANTS[mut]:
        assert _rejected((fam, name, "real"), mut), f"{fam}/{name}/real does not notice the mutant {mut}"


def test_there_are_seventeen_mutants():
    assert len(EXACT_MUTANTS) + len(REAL_MUTANTS) == 17


# ---- (a) the references against torch's own convolutions and float64 autograd ---------------------------------------------------------------

@pytest.mark.parametrize("name", list(cr.FAMILIES["fwd"]))
def test_forward_reference_agrees_with_torch(name):
    c, r = cr.case("fwd", name, "exact"), cr.ref_cpu("fwd", name, "exact")
    p, o, L = c.p, c.ops, c.Ls[0]
    w = cr.weights_of(o["wbuf"].double(), L).view(p.Cin, p.K, p.K, p.Cout).permute(3, 0, 1, 2)
    want = F.conv2d(o["x"].double(), w, o["bias"].double() if p.bias else None, stride=p.stride, padding=p.pad)
    assert bool(r.written[L.ooy::L.osc, L.oox::L.osc].all()) and int(r.written.sum()) == p.Ho * p.Wo
    assert torch.equal(want, r.ref[:, :, L.ooy::L.osc, L.oox::L.osc])          # exact operands: every float64 sum is exact


@pytest.mark.parametrize("name", list(cr.FAMILIES["tr"]))
def test_transposed_reference_agrees_with_torch(name):
    c, r = cr.case("tr", name, "exact"), cr.ref_cpu("tr", name, "exact")
    assert torch.equal(F.conv_transpose2d(c.ops["x"].double(), c.ops["w"].double(), stride=2), r.ref) and bool(r.written.all())


def test_four_scattered_products_are_the_transposed_convolution():
    cs = [cr.case("fwd", f"k1s1_scatter_{a}{b}", "exact") for a in (0, 1) for b in (0, 1)]
    p = cs[0].p
    x, wbuf = cs[0].ops["x"], cs[0].ops["wbuf"]
    y = torch.zeros((p.N, p.Cout, 2 * p.Ho, 2 * p.Wo), dtype=torch.float64)
    for c in cs:
        r = cr.assemble(x, wbuf, [SimpleNamespace(**dict(vars(c.Ls[0]), bias=0))])
        y[:, :, r.written] = r.ref[:, :, r.written]
    w = wbuf.double().view(p.Cin, 2, 2, p.Cout).permute(0, 3, 1, 2)
    assert torch.equal(F.conv_transpose2d(x.double(), w, stride=2), y)


def _layer(p, x, w):
    if p.transposed:
        return F.conv_transpose2d(x, w, stride=p.stride)
    return F.conv2d(x, w, stride=p.stride, padding=p.pad)


@pytest.mark.parametrize("name", list(cr.FAMILIES["dgrad"]))
def test_data_gradient_reference_agrees_with_autograd(name):
    c, r = cr.case("dgrad", name, "exact"), cr.ref_cpu("dgrad", name, "exact")
    p = c.p
    x = torch.zeros((p.N, p.Cin, p.H, p.W), dtype=torch.float64, requires_grad=True)
    _layer(p, x, c.ops["w"].double()).backward(c.ops["dy"].double())
    assert bool(r.written.all()) and torch.equal(x.grad, r.ref)


@pytest.mark.parametrize("name", list(cr.FAMILIES["wgrad"]))
def test_weight_gradient_reference_agrees_with_autograd(name):
    c, r = cr.case("wgrad", name, "exact"), cr.ref_cpu("wgrad", name, "exact")
    p = c.p
    w = torch.zeros(cr.weight_shape(p), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((p.Cout,), dtype=torch.float64, requires_grad=True)
    y = _layer(p, c.ops["x"].double(), w)
    if not p.transposed:
        y = y + b[None, :, None, None]
    y.backward(c.ops["dy"].double())
    assert torch.equal(w.grad, r.g)
    if not p.transposed:
        assert torch.equal(b.grad, r.db)
