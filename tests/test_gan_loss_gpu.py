"""GPU: the kernels of csrc/gan_loss.hip (weighted L1 terms, LSGAN terms, background mixing, image-pool exchange) against their host
restatements in models/gan_loss.py and against float64 torch sums. Every output is a window of a larger buffer whose rim must stay as it
was; every launch runs twice and must give the same bits."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
N_ODD = 2 * 1 * 33 * 35          # 2310: not a multiple of the eight-element vector, more than one workgroup's trip


def window(n, dtype, pad, fill=7.0):
    """(buffer, its window [pad, pad + n)): pad 8 keeps the window 16-byte aligned for both dtypes, pad 3 does not."""
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n]


def rim_intact(buf, n, pad, fill=7.0):
    return bool((buf[:pad] == fill).all() and (buf[pad + n:] == fill).all())


def grid_values(n, dtype, seed, pad=8):
    """n values on a grid of eighths (exact in both dtypes, many ties between two such tensors), in a window of the given alignment."""
    g = torch.Generator().manual_seed(seed)
    _, w = window(n, dtype, pad)
    w.copy_((torch.randint(0, 9, (n,), generator=g).float() / 8).to(dtype))
    return w


def noise_values(n, dtype, seed, pad=8):
    g = torch.Generator().manual_seed(seed)
    _, w = window(n, dtype, pad)
    w.copy_(torch.rand(n, generator=g).to(dtype))
    return w


L1_CASES = {
    "one_single_element": ([1], [3.0], 8),
    "one_odd": ([N_ODD], [10.0], 8),
    "four_unequal": ([7, 255, 256, 257], [10.0, 0.0, 0.5, 2.5], 8),
    "four_unequal_misaligned": ([N_ODD, 1, 257, 256], [1.0, 0.0, 5.0, 0.25], 3),
}


@pytest.mark.parametrize("dtypes", [(F32, F32), (BF16, BF16), (BF16, F32)], ids=["f32", "bf16", "bf16_f32"])
@pytest.mark.parametrize("case", list(L1_CASES))
def test_l1_pairs(case, dtypes, hip_lib_built):
    from octa_autosegmentation_amd.models import gan_loss
    ns, ws, pad = L1_CASES[case]
    K = len(ns)
    preds = [(noise_values if k % 2 else grid_values)(n, dtypes[0], 10 + k, pad) for k, n in enumerate(ns)]
    targets = [grid_values(n, dtypes[1], 20 + k, pad) for k, n in enumerate(ns)]
    if K > 1:
        preds[2].copy_(targets[2].to(dtypes[0]))                      # a pair that is equal everywhere
        assert ws[1] == 0.0                                          # and a zero weight
    runs = []
    for _ in range(2):
        sbuf, sums = window(K, torch.float64, 4)
        obuf, out = window(K + 1, F32, 4)
        gan_loss.l1_pairs_sums_device(preds, targets, sums)
        gan_loss.l1_pairs_finish_device(sums, ns, ws, out)
        g = torch.tensor(0.75, device="cuda")
        dwin = [window(n, dtypes[0], pad) for n in ns]
        gan_loss.l1_pairs_bwd_device(g, preds, targets, ws, [w for _, w in dwin])
        torch.cuda.synchronize()
        assert rim_intact(sbuf, K, 4) and rim_intact(obuf, K + 1, 4) and all(rim_intact(b, n, pad) for (b, _), n in zip(dwin, ns))
        runs.append((sums.clone(), out.clone(), [w.clone() for _, w in dwin]))
    sums, out, grads = runs[0]
    assert torch.equal(sums, runs[1][0]) and torch.equal(out, runs[1][1]) and all(torch.equal(a, b) for a, b in zip(grads, runs[1][2]))
    # sums: the bound of a double accumulation in any order, n * 2^-52 * sum |terms|, against a float64 torch sum over the same values
    want = gan_loss.l1_pairs_sums_host(preds, targets)
    for k in range(K):
        assert abs(float(sums[k]) - float(want[k])) <= ns[k] * 2.0 ** -52 * float(want[k]), (k, float(sums[k]), float(want[k]))
    if K > 1:
        assert float(sums[2]) == 0.0 and float(out[1]) == 0.0
    host = gan_loss.l1_pairs_finish_host(sums, ns, ws)
    assert (out - host).abs().max().item() <= 2.0 ** -23 * host.abs().max().item()          # one float32 rounding of the same double values
    for got, ref in zip(grads, gan_loss.l1_pairs_bwd_host(g, preds, targets, ws)):
        assert got.dtype == ref.dtype and torch.equal(got, ref)
    if K > 1:
        assert (grads[2] == 0).all() and (grads[1] == 0).all()      # sign(0) = 0; zero weight


def test_l1_pairs_through_autograd(hip_lib_built):
    """The public function on the device: total and terms from the kernels, the gradient through autograd; only the total carries one."""
    from octa_autosegmentation_amd.models import gan_loss
    preds = [noise_values(N_ODD, BF16, 1).view(2, 1, 33, 35).clone().requires_grad_(True), noise_values(N_ODD, BF16, 2).view(2, 1, 33, 35).clone().requires_grad_(True)]
    targets = [grid_values(N_ODD, F32, 3).view(2, 1, 33, 35), grid_values(N_ODD, F32, 4).view(2, 1, 33, 35)]
    total, terms = gan_loss.l1_pairs([(preds[0], targets[0], 10.0), (preds[1], targets[1], 5.0)])
    assert not terms.requires_grad and total.requires_grad
    (2.0 * total).backward()
    want = gan_loss.l1_pairs_bwd_host(torch.tensor(2.0, device="cuda"), [p.detach() for p in preds], targets, (10.0, 5.0))
    assert torch.equal(preds[0].grad, want[0]) and torch.equal(preds[1].grad, want[1])
    ref = sum(w * torch.nn.functional.l1_loss(p.detach().double(), t.double()) for p, t, w in zip(preds, targets, (10.0, 5.0)))
    assert abs(float(total.detach()) - float(ref)) <= 2.0 ** -22 * float(ref)
    with pytest.raises(ValueError):
        gan_loss.l1_pairs([(preds[0], targets[0], 1.0)] * 5)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shapes,pad", [([(2, 1, 2, 2)], 8), ([(3, 1, 14, 14)], 8), ([(2, 1, 2, 2), (3, 1, 14, 14)], 8), ([(3, 1, 14, 14), (2, 1, 2, 2)], 3)],
                         ids=["small", "map", "both", "both_misaligned"])
def test_lsgan(shapes, pad, dtype, hip_lib_built):
    import math
    from octa_autosegmentation_amd.models import gan_loss
    ns = [math.prod(s) for s in shapes]
    T = len(ns)
    ps = [noise_values(n, dtype, 30 + k, pad) for k, n in enumerate(ns)]
    targets, scales = (1.0, 0.0)[:T], (0.5, 0.5)[:T]
    runs = []
    for _ in range(2):
        sbuf, sums = window(T, torch.float64, 4)
        lbuf, loss = window(T + 1, F32, 4)
        gan_loss.lsgan_device(ps, targets, scales, sums, loss)
        g = torch.tensor(1.25, device="cuda")
        dwin = [window(n, dtype, pad) for n in ns]
        gan_loss.lsgan_bwd_device(g, ps, targets, scales, [w for _, w in dwin])
        torch.cuda.synchronize()
        assert rim_intact(sbuf, T, 4) and rim_intact(lbuf, T + 1, 4) and all(rim_intact(b, n, pad) for (b, _), n in zip(dwin, ns))
        runs.append((sums.clone(), loss.clone(), [w.clone() for _, w in dwin]))
    sums, loss, grads = runs[0]
    assert torch.equal(sums, runs[1][0]) and torch.equal(loss, runs[1][1]) and all(torch.equal(a, b) for a, b in zip(grads, runs[1][2]))
    want_sums, _ = gan_loss.lsgan_host(ps, targets, scales)
    for k in range(T):
        assert abs(float(sums[k]) - float(want_sums[k])) <= ns[k] * 2.0 ** -52 * float(want_sums[k]), (k, float(sums[k]), float(want_sums[k]))
    v = sums * torch.tensor(scales, dtype=torch.float64, device="cuda") / torch.tensor(ns, dtype=torch.float64, device="cuda")
    host = torch.cat((v, v.sum().reshape(1))).float()
    assert (loss - host).abs().max().item() <= 2.0 ** -23 * host.abs().max().item()
    for got, ref in zip(grads, gan_loss.lsgan_bwd_host(g, ps, targets, scales)):
        assert got.dtype == ref.dtype and torch.equal(got, ref)
    # through autograd, as the step uses it
    qs = [p.clone().view(s).requires_grad_(True) for p, s in zip(ps, shapes)]
    total, terms = gan_loss.lsgan([(q, t == 1.0, s) for q, t, s in zip(qs, targets, scales)])
    (1.25 * total).backward()
    # (the clones are aligned: for the misaligned windows the sums were taken in another order, hence one float32 rounding of slack)
    assert (torch.cat((terms, total.detach().reshape(1))) - loss).abs().max().item() <= 2.0 ** -23 * loss.abs().max().item()
    assert all(torch.equal(q.grad.view(-1), gr) for q, gr in zip(qs, grads))


def _mix_inputs(x_dtype, m_dtype, pad):
    n = N_ODD
    x, bg, u = noise_values(n, x_dtype, 40, pad), noise_values(n, m_dtype, 41, pad), noise_values(n, m_dtype, 42, pad)
    x[:700] = 0; bg[:400] = 0; u[300:600] = 0                        # zeros against zeros: exact ties (the empty background of a rasterised graph)
    x[1000:1500] = -1.0                                              # a stretch with x < m throughout
    return x, bg, u


@pytest.mark.parametrize("pad", [8, 3], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("x_dtype,m_dtype", [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)], ids=["f32", "bf16", "bf16_x", "bf16_m"])
def test_mix_max(x_dtype, m_dtype, pad, hip_lib_built):
    from octa_autosegmentation_amd.models import gan_loss
    x, bg, u = _mix_inputs(x_dtype, m_dtype, pad)
    n = x.numel()
    o_dtype = BF16 if x_dtype == BF16 and m_dtype == BF16 else F32
    dout = noise_values(n, o_dtype, 43, pad)
    runs = []
    for _ in range(2):
        obuf, out = window(n, o_dtype, pad)
        dbuf, dx = window(n, x_dtype, pad)
        gan_loss.mix_max_device(x, bg, u, out)
        gan_loss.mix_max_bwd_device(x, bg, u, dout, dx)
        torch.cuda.synchronize()
        assert rim_intact(obuf, n, pad) and rim_intact(dbuf, n, pad)
        runs.append((out.clone(), dx.clone()))
    out, dx = runs[0]
    assert torch.equal(out, runs[1][0]) and torch.equal(dx, runs[1][1])
    want = torch.maximum(x, bg * u)                                  # float32: torch's own expression; bf16: the same, which is the restatement
    assert want.dtype == out.dtype and torch.equal(out, want) and torch.equal(out, gan_loss.mix_max_host(x, bg, u))
    ref = gan_loss.mix_max_bwd_host(x, bg, u, dout)
    assert ref.dtype == dx.dtype and torch.equal(dx, ref)
    m = (bg * u).float()
    tie = x.float() == m
    assert tie.sum() >= 400 and torch.equal(dx[tie].float(), (0.5 * dout[tie].float()).to(x_dtype).float())
    assert (dx[1000:1500] == 0).all() and (x.float() > m).any()
    # all of x below m: no gradient at all
    low = torch.full_like(x, -2.0)
    assert (gan_loss.mix_max_bwd_device(low, bg, u, dout) == 0).all()
    # through autograd
    xr = x.clone().requires_grad_(True)
    gan_loss.mix_max(xr, bg, u).backward(dout)
    assert torch.equal(xr.grad, dx)


POOL_TABLES = {
    # pool_size, (src, wslot, winput) for a batch of three
    "two_on_one_slot": (3, ([-1 - 1, 0, 2], [1], [1])),
    "three_on_one_slot": (3, ([-1 - 0, 0, 1], [0], [2])),
    "pool_of_one": (1, ([-1, 0, 1], [0], [2])),
    "pool_of_one_two_draws": (1, ([0, -1, 1], [0], [2])),
    "append_and_exchange": (3, ([0, 0, -1 - 0], [2, 0], [1, 2])),      # image 0 fills slot 2, image 1 draws slot 2, image 2 draws slot 0
    "nothing_drawn": (3, ([0, 1, 2], [], [])),
}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("plane", [(1, 5, 7), (1, 8, 8)], ids=["5x7", "8x8"])
@pytest.mark.parametrize("case", list(POOL_TABLES))
def test_pool_exchange_tables(case, plane, dtype, hip_lib_built):
    """One launch against the host restatement on resolved tables; 5 x 7 planes are no multiple of any vector width (and their rows start
    at odd offsets), 8 x 8 planes take the 16-byte path."""
    import math
    from octa_autosegmentation_amd.models import gan_loss
    P, tables = POOL_TABLES[case]
    E, B, pad = math.prod(plane), 3, 8
    g = torch.Generator().manual_seed(5)
    old = torch.rand((P,) + plane, generator=g).to(dtype).cuda()
    images = torch.rand((B,) + plane, generator=g).to(dtype).cuda()
    host_pool = old.clone()
    want = gan_loss.pool_exchange_host(host_pool, images, *tables)
    for _ in range(2):
        pbuf, pool = window(P * E, dtype, pad)
        pool.copy_(old.view(-1))
        obuf, out = window(B * E, dtype, pad)
        gan_loss.pool_exchange_device(pool.view((P,) + plane), images, *tables, out=out.view((B,) + plane))
        torch.cuda.synchronize()
        assert rim_intact(pbuf, P * E, pad) and rim_intact(obuf, B * E, pad)
        assert torch.equal(out.view((B,) + plane), want) and torch.equal(pool.view((P,) + plane), host_pool)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pool_size", [1, 3])
def test_image_pool_on_the_device_equals_the_host_pool(pool_size, dtype, hip_lib_built):
    """ImagePool with device tensors against ImagePool with CPU tensors, the same seed: every returned batch and the final pool equal;
    the sequence must contain a batch that fills and exchanges at once and batches where one slot is drawn twice."""
    from octa_autosegmentation_amd.models.cycle_gan import ImagePool
    g = torch.Generator().manual_seed(6)
    batches = [torch.rand(3, 1, 5, 7, generator=g).to(dtype) for _ in range(12)]
    random.seed(3)
    host = ImagePool(pool_size)
    want = [host.query(b) for b in batches]
    random.seed(3)
    probe = ImagePool(pool_size)
    tables = [probe.resolve(3) for _ in batches]
    assert any(any(0 <= s != k for k, s in enumerate(src)) for src, _, _ in tables)       # an image received an earlier image of its own batch
    random.seed(3)
    dev = ImagePool(pool_size)
    got = [dev.query(b.cuda()) for b in batches]
    torch.cuda.synchronize()
    assert dev.images.is_cuda and dev.images.dtype == dtype and dev.images.shape == (pool_size, 1, 5, 7)
    for a, b in zip(got, want):
        assert a.dtype == dtype and torch.equal(a.cpu(), b)
    assert torch.equal(dev.images.cpu(), host.images)


def test_bad_arguments_are_refused_before_any_launch(hip_lib_built):
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import gan_loss
    pool, images = torch.zeros(2, 1, 5, 7, device="cuda"), torch.zeros(3, 1, 5, 7, device="cuda")
    for tables in (([3, 0, 1], [], []), ([-3, 0, 1], [], []), ([0, 1, 2], [2], [0]), ([0, 1, 2], [0], [3]), ([0, 1, 2], [1, 1], [0, 2])):
        with pytest.raises(_native.OctaHipError):
            gan_loss.pool_exchange_device(pool, images, *tables)
    with pytest.raises(TypeError):
        gan_loss.mix_max_device(images.half(), images.half(), images.half())
