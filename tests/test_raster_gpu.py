"""GPU parity: the HIP rasteriser / dither through the C-ABI vs the oracle and the golden fixtures."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2i(hip_lib_built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from octa_autosegmentation_amd.vessel_graph_generation import tree2img
    return tree2img


def dev_raster(t2i, edges_list, res, mip=2, minr=-np.inf, maxr=np.inf, keep=None):
    import torch
    off = np.zeros(len(edges_list) + 1, np.int64)
    off[1:] = np.cumsum([len(e) for e in edges_list])
    cat = np.concatenate([np.asarray(e, np.float64).reshape(-1, 7) for e in edges_list]) if off[-1] else np.zeros((0, 7))
    d = torch.from_numpy(cat).cuda()
    dk = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).cuda() if keep is not None else None
    out = t2i.rasterize_edges_device(d, off, res, mip, minr, maxr, dk)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_full_graphs_bit_exact(t2i, raster_golden):
    g = raster_golden
    e0, e1 = g["graph0_edges"], g["graph1_edges"]
    out = dev_raster(t2i, [e0, e1], [304, 304])
    assert (out[0] == g["graph0_img304"]).all() and (out[1] == g["graph1_img304"]).all()
    out = dev_raster(t2i, [e0, e1], [1216, 1216])
    assert (out[0] == g["graph0_img1216"]).all() and (out[1] == g["graph1_img1216"]).all()
    out = dev_raster(t2i, [e0], [1216, 1216], minr=0.0033, maxr=1.0)
    assert hashlib.sha256(out[0].tobytes()).hexdigest() == str(g["graph0_img1216_minr_sha256"])


def test_plan_and_draw_are_the_two_halves_of_one_call(t2i, raster_golden):
    """octa_rasterize_2d_plan / _draw (pipeline.py plans two rasterisations while the GPU is free and draws them later): two plans on two
    contexts, drawn in the other order, give the golden images; a context holds one plan and a draw consumes it."""
    import torch
    from octa_autosegmentation_amd import _native
    g = raster_golden
    e0, e1 = np.asarray(g["graph0_edges"], np.float64), np.asarray(g["graph1_edges"], np.float64)
    off = np.array([0, len(e0), len(e0) + len(e1)], np.int64)
    d = torch.from_numpy(np.concatenate([e0, e1])).cuda()
    a, b = _native.new_ctx(), _native.new_ctx()
    try:
        with _native.use_ctx(a):
            p_small = t2i.rasterize_edges_device_plan(d, off, [304, 304])
        with _native.use_ctx(b):
            p_large = t2i.rasterize_edges_device_plan(d, off, [1216, 1216])
        del d                                           # the plans hold everything the draws read
        torch.cuda.empty_cache()
        large = t2i.rasterize_edges_device_draw(p_large).cpu().numpy()
        small = t2i.rasterize_edges_device_draw(p_small).cpu().numpy()
        assert (small[0] == g["graph0_img304"]).all() and (small[1] == g["graph1_img304"]).all()
        assert (large[0] == g["graph0_img1216"]).all() and (large[1] == g["graph1_img1216"]).all()
        with pytest.raises(_native.OctaHipError, match="no plan"):
            t2i.rasterize_edges_device_draw(p_small)    # consumed
    finally:
        _native.free_ctx(a)
        _native.free_ctx(b)


def _other_calls(t2i):
    """name -> a call of another module on the calling thread's context (small seeded inputs), returning its result tensors. Between
    them they take every work buffer the draw half uses, and the voxeliser's per-edge index besides."""
    import torch
    from octa_autosegmentation_amd import _native, graph_io
    from octa_autosegmentation_amd.models import postprocess
    from octa_autosegmentation_amd.utils import skeleton
    rng = np.random.default_rng(7)
    vox_edges = torch.from_numpy(np.array([[0.2, 0.2, 0.2, 0.7, 0.6, 0.5, 0.06], [0.1, 0.8, 0.3, 0.6, 0.2, 0.7, 0.05],
                                           [0.5, 0.5, 0.1, 0.5, 0.5, 0.9, 0.08]])).cuda()
    vol = torch.from_numpy((rng.random((1, 4, 8, 8)) > 0.5).astype(np.uint8)).cuda()
    img = torch.from_numpy((rng.random((1, 8, 8)) > 0.4).astype(np.uint8)).cuda()
    x = torch.from_numpy(rng.standard_normal((1, 2, 64)).astype(np.float32)).cuda()
    rows = torch.from_numpy(rng.random((3, 7))).cuda()

    def instnorm():
        y, mean, rstd = torch.empty_like(x), torch.empty(2, device="cuda"), torch.empty(2, device="cuda")
        _native.launch("octa_instnorm_lrelu_fwd", x.device, x, y, None, None, mean, rstd, 1, 2, 64, 0, 0.01, 1e-5)
        return y, mean, rstd

    return {
        "voxelize_edges_device": lambda: (t2i.voxelize_edges_device(vox_edges, np.array([0, 1, 3]), [8, 8, 8]),),
        "octa_cc3d_filter": lambda: postprocess.cc3d_filter_device(vol, 3, 0, min_size=3, return_info=True),
        "octa_remove_small_objects": lambda: (postprocess.remove_small_objects_device(img, min_size=3),),
        "octa_skeletonize": lambda: (skeleton.skeletonize_device(img),),
        "octa_instnorm_lrelu_fwd": instnorm,
        "edges_as_read_back_device": lambda: (graph_io.edges_as_read_back_device(rows),),
    }


OTHER_CALLS = ["voxelize_edges_device", "octa_cc3d_filter", "octa_remove_small_objects", "octa_skeletonize", "octa_instnorm_lrelu_fwd",
               "edges_as_read_back_device"]


@pytest.mark.parametrize("other", OTHER_CALLS)
def test_other_calls_between_plan_and_draw_leave_the_plan_intact(t2i, raster_golden, other):
    """A context holds one plan, and any other entry point may run on it between plan and draw (include/octa_hip.h): graph 0 has
    13 821 edges, so four scan blocks whose bases are not all zero, and the draw after the other call gives the golden image bit for
    bit; the other call gives what it gives on a fresh context."""
    import torch
    from octa_autosegmentation_amd import _native
    e0 = np.asarray(raster_golden["graph0_edges"], np.float64)
    assert len(e0) > 3 * 4096
    d = torch.from_numpy(e0).cuda()
    call = _other_calls(t2i)[other]
    fresh, held = _native.new_ctx(), _native.new_ctx()
    try:
        with _native.use_ctx(fresh):
            want = [t.cpu() for t in call()]
        with _native.use_ctx(held):
            plan = t2i.rasterize_edges_device_plan(d, np.array([0, len(e0)]), [304, 304])
            got = [t.cpu() for t in call()]
            out = t2i.rasterize_edges_device_draw(plan).cpu().numpy()
        assert (out[0] == raster_golden["graph0_img304"]).all()
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        _native.free_ctx(fresh)
        _native.free_ctx(held)


def test_scratch_bytes_counts_every_buffer_and_reaches_a_steady_state(t2i, raster_golden):
    """octa_ctx_scratch_bytes counts everything the context holds (0 when fresh, the norm kernels' ring of pre-zeroed slots -- 4 MiB at
    least -- after one channels-last norm without statistics from outside), and no buffer grows on a second call of the same shapes."""
    import torch
    from octa_autosegmentation_amd import _native
    held = lambda: _native.lib().octa_ctx_scratch_bytes(h)
    e0 = np.asarray(raster_golden["graph0_edges"], np.float64)
    d = torch.from_numpy(e0).cuda()
    calls = _other_calls(t2i)
    h = _native.new_ctx()
    try:
        assert held() == 0
        with _native.use_ctx(h):
            x = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 8, 8, 32)).astype(np.float32)).cuda().to(torch.bfloat16)
            y, mean, rstd = torch.empty_like(x), torch.empty(32, device="cuda"), torch.empty(32, device="cuda")
            _native.launch("octa_instnorm_lrelu_nhwc_fwd", x.device, x, y, None, None, mean, rstd, 1, 32, 64, 0.01, 1e-5, None, 0, None, 0)
            assert held() >= 4 << 20
            rounds = []
            for _ in range(3):
                plan = t2i.rasterize_edges_device_plan(d, np.array([0, len(e0)]), [304, 304])
                for name in OTHER_CALLS:
                    calls[name]()
                t2i.rasterize_edges_device_draw(plan)
                rounds.append(held())
            torch.cuda.synchronize()
        assert rounds[0] == rounds[1] == rounds[2]
    finally:
        _native.free_ctx(h)


def test_labels_bit_exact(t2i, raster_golden):
    import torch
    g = raster_golden
    d = torch.from_numpy(np.stack([g["graph0_img1216"], g["graph1_img1216"]])).cuda()
    out = t2i.binarize_label_device(d).cpu().numpy()
    for k in range(2):
        label = np.unpackbits(g[f"graph{k}_label_packed"])[: 1216 * 1216].reshape(1216, 1216) * 255
        assert (out[k] == label).all()


def test_18_shipped_labels_bit_exact_in_one_ragged_batch(t2i, raster_golden):
    """The reference's shipped csv <-> label pairs (round-4 verdict item 5): raster_golden.npz's two + the 16 of
    tests/golden/raster_shipped_golden.npz (tools/make_golden_raster_shipped.py) as ONE ragged batch (13.2 k - 14.3 k edges each) through
    octa_rasterize_2d at 1216 x 1216 and octa_fs_dither: every label PNG bit for bit, every 304 x 304 / 1216 x 1216 raster by its SHA-256."""
    import os
    import torch
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "raster_shipped_golden.npz"))
    n = len(g["names"])
    assert n >= 16
    edges = [raster_golden["graph0_edges"], raster_golden["graph1_edges"]] + [g[f"edges_{k}"] for k in range(n)]
    grey = dev_raster(t2i, edges, [1216, 1216])
    small = dev_raster(t2i, edges, [304, 304])
    bits = t2i.binarize_label_device(torch.from_numpy(grey).cuda()).cpu().numpy()
    for k in range(2):
        assert (grey[k] == raster_golden[f"graph{k}_img1216"]).all() and (small[k] == raster_golden[f"graph{k}_img304"]).all()
        assert (bits[k] == np.unpackbits(raster_golden[f"graph{k}_label_packed"])[: 1216 * 1216].reshape(1216, 1216) * 255).all()
    for k in range(n):
        name = str(g["names"][k])
        assert hashlib.sha256(grey[2 + k].tobytes()).hexdigest() == str(g[f"img1216_sha256_{k}"]), name
        assert hashlib.sha256(small[2 + k].tobytes()).hexdigest() == str(g[f"img304_sha256_{k}"]), name
        label = np.unpackbits(g[f"label_packed_{k}"])[: 1216 * 1216].reshape(1216, 1216) * 255
        assert (bits[2 + k] == label).all(), name


def test_synthetic_cases(t2i, raster_golden):
    g = raster_golden
    for t in range(int(g["n_syn"])):
        W, H, mip = (int(v) for v in g[f"syn{t}_res"])
        out = dev_raster(t2i, [g[f"syn{t}_edges"]], [W, H], mip)
        assert (out[0] == g[f"syn{t}_img"]).all(), f"synthetic case {t}"


def test_fs_dither_cases(t2i, raster_golden):
    import torch
    g = raster_golden
    for t in range(int(g["n_fs"])):
        d = torch.from_numpy(g[f"fs{t}_in"][None].copy()).cuda()
        out = t2i.binarize_label_device(d).cpu().numpy()[0]
        assert (out == g[f"fs{t}_out"]).all(), f"fs case {t}"


def test_fs_dither_random_images_of_odd_sizes_match_the_oracle(t2i):
    """Widths that are no multiples of 4 / 16, heights that leave a ragged last band of the 64-row wavefront, one-pixel and one-row
    images, batches, and a full-size noise image (every error term alive, unlike the mostly black labels)."""
    import torch
    from oracle import octa_oracle
    rng = np.random.default_rng(5)
    for (B, H, W) in [(1, 1, 1), (2, 1, 7), (1, 9, 1), (3, 5, 3), (2, 64, 64), (2, 65, 66), (1, 200, 65), (2, 130, 67), (1, 129, 304), (1, 1216, 1216)]:
        x = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        if H * W > 10000:
            x[0, : H // 2] = np.minimum(x[0, : H // 2], 140)          # a band around the threshold: long carry chains
        out = t2i.binarize_label_device(torch.from_numpy(x).cuda()).cpu().numpy()
        for b in range(B):
            assert (out[b] == octa_oracle.fs_dither(x[b])).all(), (B, H, W, b)


def test_fs_dither_pipeline_of_waves_matches_the_oracle_and_the_one_wave_kernel(t2i, monkeypatch):
    """Round 4: images whose rows are 16-byte aligned take the pipelined kernel (bands of 64 rows on the waves of one workgroup, error
    rows handed over through LDS): 2 to 19+ bands, ragged last bands, more bands than waves (17 x 64 + 5 rows), batches, noise that keeps
    every error term alive -- all equal to the oracle, and to the one-wave kernel (OCTA_DITHER_PIPE is read once per process, so the
    one-wave kernel is reached through a width that is no multiple of 16)."""
    import torch
    from oracle import octa_oracle
    rng = np.random.default_rng(17)
    for (B, H, W) in [(2, 65, 64), (3, 128, 304), (1, 129, 16), (2, 200, 320), (1, 1093, 1216), (2, 1216, 1216), (1, 1300, 608)]:
        x = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        x[0, : H // 2] = np.minimum(x[0, : H // 2], 140)
        if B > 1:
            x[1] = (rng.random((H, W)) < 0.1) * rng.integers(1, 256, (H, W))      # mostly black, like a label
        out = t2i.binarize_label_device(torch.from_numpy(x).cuda()).cpu().numpy()
        for b in range(B):
            assert (out[b] == octa_oracle.fs_dither(x[b])).all(), (B, H, W, b)
    # same picture through both kernels: pad a 16-aligned image by one column of zeros on the right (the extra column only receives error)
    x = rng.integers(0, 256, (1, 300, 304), dtype=np.uint8)
    a = t2i.binarize_label_device(torch.from_numpy(x).cuda()).cpu().numpy()[0]
    xp = np.concatenate([x, np.zeros((1, 300, 1), np.uint8)], axis=2)
    bq = t2i.binarize_label_device(torch.from_numpy(np.ascontiguousarray(xp)).cuda()).cpu().numpy()[0]
    assert (bq == octa_oracle.fs_dither(xp[0])).all() and (a == octa_oracle.fs_dither(x[0])).all()


def test_random_vs_oracle_and_ragged_batch(t2i):
    from oracle import octa_oracle
    rng = np.random.default_rng(99)
    graphs = []
    for b in range(9):
        n = [0, 1, 5, 300, 2000, 17, 0, 64, 4097][b]
        e = np.zeros((n, 7))
        e[:, 0:3] = rng.uniform(-0.1, 1.1, (n, 3))
        d = rng.normal(0, 0.03, (n, 3))
        e[:, 3:6] = e[:, 0:3] + d
        e[:, 6] = rng.uniform(0.0008, 0.012, n)
        graphs.append(e)
    for res in ([304, 304], [200, 120], [65, 190]):
        out = dev_raster(t2i, graphs, res)
        for b, e in enumerate(graphs):
            ref = octa_oracle.rasterize(e, res)
            assert (out[b] == ref).all(), (res, b)
    keep = (rng.random(len(graphs[4])) < 0.5).astype(np.uint8)
    out = dev_raster(t2i, [graphs[4]], [304, 304], keep=keep)
    assert (out[0] == octa_oracle.rasterize(graphs[4], [304, 304], keep=keep)).all()


def test_dense_tile_chunking(t2i):
    """More edges through one 64x64 tile than one LDS chunk holds: the ordered chunk hand-over."""
    from oracle import octa_oracle
    rng = np.random.default_rng(3)
    n = 6000
    e = np.zeros((n, 7))
    e[:, 0:2] = rng.uniform(0.3, 0.5, (n, 2))
    e[:, 3:5] = e[:, 0:2] + rng.normal(0, 0.05, (n, 2))
    e[:, 6] = rng.uniform(0.0005, 0.004, n)
    out = dev_raster(t2i, [e], [256, 256])
    assert (out[0] == octa_oracle.rasterize(e, [256, 256])).all()
    # very wide strokes (many cap vertices per edge)
    e2 = e[:40].copy()
    e2[:, 6] = rng.uniform(0.05, 0.4, 40)
    out = dev_raster(t2i, [e2], [256, 256])
    assert (out[0] == octa_oracle.rasterize(e2, [256, 256])).all()


def test_rasterize_forest_signature_and_dropout(t2i, raster_golden):
    g = raster_golden
    e = g["drop_edges"]
    forest = [{"node1": e[i, 0:3].copy(), "node2": e[i, 3:6].copy(), "radius": e[i, 6]} for i in range(len(e))]
    random.seed(1234)
    rl = []
    img_a, bd = t2i.rasterize_forest(forest, [304, 304], 2, radius_list=rl, max_dropout_prob=1.0)
    assert random.random() == float(g["drop_next_random"])
    assert img_a.dtype == np.uint16 and (img_a == g["drop_img_a"]).all()
    img_b, bd2 = t2i.rasterize_forest(forest, [608, 608], 2, min_radius=0.002, blackdict=bd)
    assert (img_b == g["drop_img_b"]).all() and len(bd2) == int(g["drop_n_black"])
    # legacy string positions (the CSV read-back path, tree2img.py:73-76)
    forest_s = [{"node1": str(e[i, 0:3]), "node2": str(e[i, 3:6]), "radius": repr(float(e[i, 6]))} for i in range(200)]
    from oracle import octa_oracle
    img_s, _ = t2i.rasterize_forest(forest_s, [304, 304])
    p = lambda s: [float(c) for c in s[1:-1].split(" ") if len(c) > 0]
    es = np.array([p(r["node1"]) + p(r["node2"]) + [float(r["radius"])] for r in forest_s])
    assert (img_s == octa_oracle.rasterize(es, [304, 304])).all()


def test_max_u8(t2i):
    import torch
    a = torch.randint(0, 256, (3, 77, 91), dtype=torch.uint8, device="cuda")
    b = torch.randint(0, 256, (3, 77, 91), dtype=torch.uint8, device="cuda")
    assert torch.equal(t2i.maximum_u8_device(a, b), torch.maximum(a, b))


def test_label_bits_packed_on_the_device_are_numpys_packbits(t2i):
    """octa_pack_bits: the mode "1" rows of binarised labels (visualize_vessel_graphs.py:99), bit 7 of a byte = its first pixel, for widths
    that are and are not multiples of eight and values that are merely non-zero."""
    import torch
    for shape in ((2, 1216, 1216), (3, 37, 53), (1, 5, 8), (2, 9, 131)):
        a = torch.randint(0, 3, shape, dtype=torch.uint8, device="cuda") * 127        # 0, 127, 254: non-zero = white
        got = t2i.pack_label_bits_device(a).cpu().numpy()
        assert got.shape == (shape[0], shape[1], (shape[2] + 7) // 8)
        assert (got == np.packbits(a.cpu().numpy() > 0, axis=2)).all()
