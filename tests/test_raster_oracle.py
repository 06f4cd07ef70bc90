"""CPU: pins the raster/dither oracle against fixtures produced by the reference itself
(tools/make_golden_raster.py: matplotlib Agg via the reference's rasterize_forest, Pillow
convert("1"), and the reference's shipped label PNGs)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import octa_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_full_graphs(raster_golden):
    g = raster_golden
    for k in range(int(g["n_graphs"])):
        e = g[f"graph{k}_edges"]
        assert (octa_oracle.rasterize(e, [304, 304]) == g[f"graph{k}_img304"]).all()
        img = octa_oracle.rasterize(e, [1216, 1216])
        assert (img == g[f"graph{k}_img1216"]).all()
        f = octa_oracle.rasterize(e, [1216, 1216], min_radius=0.0033, max_radius=1)
        assert hashlib.sha256(f.tobytes()).hexdigest() == str(g[f"graph{k}_img1216_minr_sha256"])
        # label = Floyd-Steinberg of the raster == the PNG shipped in the reference's datasets/labels
        label = np.unpackbits(g[f"graph{k}_label_packed"])[: 1216 * 1216].reshape(1216, 1216) * 255
        assert (octa_oracle.fs_dither(img) == label).all()


def test_oracle_synthetic(raster_golden):
    g = raster_golden
    for t in range(int(g["n_syn"])):
        W, H, mip = (int(v) for v in g[f"syn{t}_res"])
        img = octa_oracle.rasterize(g[f"syn{t}_edges"], [W, H], mip)
        assert img.shape == g[f"syn{t}_img"].shape
        assert (img == g[f"syn{t}_img"]).all(), f"synthetic case {t}"


def test_oracle_fs_dither(raster_golden):
    g = raster_golden
    for t in range(int(g["n_fs"])):
        assert (octa_oracle.fs_dither(g[f"fs{t}_in"]) == g[f"fs{t}_out"]).all()


def test_oracle_edge_cases():
    # empty graph, fully-outside edge, zero-length edge, radius window
    assert octa_oracle.rasterize(np.zeros((0, 7)), [32, 24]).sum() == 0
    e = np.array([[2.0, 2.0, 0, 3.0, 3.0, 0, 0.01], [0.5, 0.5, 0, 0.5, 0.5, 0, 0.01]])
    assert octa_oracle.rasterize(e, [32, 24]).sum() == 0
    e = np.array([[0.2, 0.2, 0, 0.8, 0.8, 0, 0.01]])
    assert octa_oracle.rasterize(e, [32, 32]).sum() > 0
    assert octa_oracle.rasterize(e, [32, 32], min_radius=0.02, max_radius=1).sum() == 0
    keep = np.array([0], np.uint8)
    assert octa_oracle.rasterize(e, [32, 32], keep=keep).sum() == 0


def test_kernel_arithmetic_on_host(raster_golden):
    """The HIP kernel's closed-form cell evaluation (csrc/raster_core.h compiled as host C++)
    against the golden images: catches kernel-math regressions without a GPU."""
    import ctypes
    src = os.path.join(ROOT, "tests", "native", "raster_core_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libcorehost.so")
    hdr = os.path.join(ROOT, "octa_autosegmentation_amd", "csrc", "raster_core.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    ch = ctypes.CDLL(so)
    ch.octa_corehost_rasterize.restype = ctypes.c_long
    ch.octa_corehost_rasterize.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]

    def core(e, W, H, mip=2):
        e = np.ascontiguousarray(e, dtype=np.float64)
        out = np.zeros((H, W), np.uint8)
        n = ch.octa_corehost_rasterize(e.ctypes.data, len(e), W, H, mip, -np.inf, np.inf, None, out.ctypes.data)
        assert n >= 0
        return out

    ch.octa_corehost_rasterize_acc.restype = ctypes.c_long
    ch.octa_corehost_rasterize_acc.argtypes = ch.octa_corehost_rasterize.argtypes

    def core_acc(e, W, H, mip=2):
        """the item-parallel form of the fold (round 4): pieces walked cell by cell into per-block accumulators (hline_cells)"""
        e = np.ascontiguousarray(e, dtype=np.float64)
        out = np.zeros((H, W), np.uint8)
        n = ch.octa_corehost_rasterize_acc(e.ctypes.data, len(e), W, H, mip, -np.inf, np.inf, None, out.ctypes.data)
        assert n >= 0
        return out

    g = raster_golden
    for t in range(int(g["n_syn"])):
        W, H, mip = (int(v) for v in g[f"syn{t}_res"])
        assert (core(g[f"syn{t}_edges"], W, H, mip) == g[f"syn{t}_img"]).all(), f"synthetic case {t}"
        assert (core_acc(g[f"syn{t}_edges"], W, H, mip) == g[f"syn{t}_img"]).all(), f"synthetic case {t} (accumulator form)"
    assert (core(g["graph0_edges"], 304, 304) == g["graph0_img304"]).all()
    assert (core(g["graph1_edges"], 1216, 1216) == g["graph1_img1216"]).all()
    assert (core_acc(g["graph0_edges"], 304, 304) == g["graph0_img304"]).all()
    assert (core_acc(g["graph1_edges"], 1216, 1216) == g["graph1_img1216"]).all()


def test_oracle_reproduces_16_more_shipped_pairs():
    """tests/golden/raster_shipped_golden.npz (tools/make_golden_raster_shipped.py): 16 further csv <-> label pairs the reference ships
    (datasets/vessel_graphs/*.csv <-> datasets/labels/*.png), as data: edge array, the shipped label's bits, SHA-256 of the reference's own
    304 x 304 and 1216 x 1216 rasters. The oracle must reproduce all of them; with raster_golden.npz's two that is 18 shipped labels."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "raster_shipped_golden.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) >= 16
    for k, name in enumerate(names):
        e = g[f"edges_{k}"]
        assert hashlib.sha256(octa_oracle.rasterize(e, [304, 304]).tobytes()).hexdigest() == str(g[f"img304_sha256_{k}"]), name
        img = octa_oracle.rasterize(e, [1216, 1216])
        assert hashlib.sha256(img.tobytes()).hexdigest() == str(g[f"img1216_sha256_{k}"]), name
        label = np.unpackbits(g[f"label_packed_{k}"])[: 1216 * 1216].reshape(1216, 1216) * 255
        assert (octa_oracle.fs_dither(img) == label).all(), name


def _decode_sample_graph(g, k):
    """Edge array [n, 7] of graph k of raster_labels_sample_golden (tools/make_golden_raster_labels_sample.py): node coordinates as
    printed in the CSV (mantissa * 10**exponent), a node stored as its difference to its parent at its own exponent; exact integers in
    units of 1e-16, so every double equals float() of the CSV token."""
    delta, x, parent, ends = g[f"delta_{k}"], g[f"exp_{k}"], g[f"parent_{k}"], g[f"ends_{k}"]
    v = [None] * len(delta)
    for j in range(len(delta)):
        v[j] = [(int(d) + (v[int(parent[j])][c] // 10 ** (16 + int(e)) if parent[j] >= 0 else 0)) * 10 ** (16 + int(e))
                for c, (d, e) in enumerate(zip(delta[j], x[j]))]
    nodes = np.array([[float(f"{a}e-16") for a in p] for p in v])
    return np.concatenate([nodes[ends[:, 0]], nodes[ends[:, 1]], g[f"radii_{k}"][g[f"radius_index_{k}"]][:, None]], axis=1)


def test_oracle_reproduces_shipped_labels_sample():
    """A spread of the 500 shipped csv<->label pairs: every 100th of the sorted list. Two of the five are held by raster_golden.npz and
    raster_shipped_golden.npz (edges, label bits); the other three by raster_labels_sample_golden.npz.xz (edges, SHA-256 of the
    label's pixels). tools/make_golden_raster_labels_sample.py checks that both hold exactly the shipped files' contents."""
    import io
    import lzma
    with open(os.path.join(ROOT, "tests", "golden", "raster_labels_sample_golden.npz.xz"), "rb") as f:
        g = np.load(io.BytesIO(lzma.decompress(f.read())))
    names = [str(n) for n in g["names"]]
    new = [str(n) for n in g["new_names"]]
    held = {}
    r = np.load(os.path.join(ROOT, "tests", "golden", "raster_golden.npz"))
    held[str(r["graph0_name"])] = (r["graph0_edges"], r["graph0_label_packed"])
    s = np.load(os.path.join(ROOT, "tests", "golden", "raster_shipped_golden.npz"))
    for k, n in enumerate(s["names"]):
        held[str(n)] = (s[f"edges_{k}"], s[f"label_packed_{k}"])
    assert len(names) == 5 and set(names) <= set(new) | set(held)
    for fn in names:
        if fn in new:
            k = new.index(fn)
            lab = octa_oracle.fs_dither(octa_oracle.rasterize(_decode_sample_graph(g, k), [1216, 1216]))
            assert hashlib.sha256(np.ascontiguousarray(lab, np.uint8).tobytes()).hexdigest() == str(g[f"label_sha256_{k}"]), fn
        else:
            e, bits = held[fn]
            label = np.unpackbits(bits)[: 1216 * 1216].reshape(1216, 1216) * 255
            assert (octa_oracle.fs_dither(octa_oracle.rasterize(e, [1216, 1216])) == label).all(), fn
