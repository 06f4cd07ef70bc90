"""GPU time of the 3-D connected-component filter (csrc/cc3d.hip) on three masks of 44 x 1216 x 1216 voxels, the volume
configs/config_3d_recon_supervised.yml predicts:

  (a) a thresholded random field at 8 % density with the central depth plane filled (what RemoveOuterNoise hands to the kernel);
  (b) the same field without the plane;
  (c) the rasteriser fixture's graph, voxelised at 1216 x 1216 x 16 and cut to the 44 slices SelectSlice keeps, plus 2 % salt noise,
      plane filled.

For each: octa_cc3d_filter at connectivity 3, mode 1 (largest component) and mode 0 (min_size 16), ms per call and voxels/s; the HBM
bytes its passes touch BY COUNT (hbm_bytes below: computed from the shape and the mask, not measured) and that over the time as a
fraction of 8 TB/s; the per-slice filter octa_remove_small_objects at B = 44 on the same mask in the same run, alternating with it;
and the scipy restatement (ndimage.label + bincount + argmax) on one CPU core, once, whose result the kernel's must equal.

Host clock around work that ends in a device synchronise; every mask is warmed up first. Run by hand; nothing here is gated."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from octa_autosegmentation_amd.models import postprocess  # noqa: E402

SHAPE = (44, 1216, 1216)
BRICK = (4, 8, 64)          # BZ, BY, BX of csrc/cc3d.hip
HBM_PEAK = 8e12


def timed(f, n):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def seam_neighbours(connectivity):
    """(fraction of a brick's voxels on its faces, mean number of forward neighbours outside the brick per face voxel)."""
    bz, by, bx = BRICK
    z, y, x = np.indices(BRICK)
    face = (z == 0) | (z == bz - 1) | (y == 0) | (y == by - 1) | (x == 0) | (x == bx - 1)
    out = np.zeros(BRICK, np.int64)
    for dz in (0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) > (0, 0, 0) and dz + abs(dy) + abs(dx) <= connectivity:
                    out += (z + dz >= bz) | (y + dy < 0) | (y + dy >= by) | (x + dx < 0) | (x + dx >= bx)
    return face.mean(), out[face].mean()


def hbm_bytes(mask, connectivity, mode):
    """Bytes the passes of csrc/cc3d.hip read and write, counted from the shape and the foreground (every access once: what the caches
    absorb -- root walks, the neighbour labels a face voxel shares with the next one -- is not subtracted and not added twice):
    local   1 B in + 4 B label per voxel, 4 B count per foreground voxel
    seam    4 B own label per face voxel, 4 B per foreground face voxel and forward neighbour outside the brick
    resolve 4 B label per voxel; per foreground voxel 4 B root's label, 4 B label written, 4 B count
    roots   4 B label per voxel (mode 1)
    filter  4 B label + 1 B out per voxel, 4 B root's count per foreground voxel (mode 0)"""
    n, fg = mask.size, int(np.count_nonzero(mask))
    face, cross = seam_neighbours(connectivity)
    local = 5 * n + 4 * fg
    seam = 4 * face * n + 4 * cross * face * fg
    resolve = 4 * n + 12 * fg
    roots = 4 * n if mode == 1 else 0
    filt = 5 * n + (4 * fg if mode == 0 else 0)
    return local + seam + resolve + roots + filt


def fixture_volume():
    """graph0 of tests/golden/raster_golden.npz voxelised at 1216 x 1216 x 16 (padded to Z = 53), depth first, slices 5 .. -4."""
    from octa_autosegmentation_amd.vessel_graph_generation import tree2img
    e = np.load(os.path.join(ROOT, "tests", "golden", "raster_golden.npz"))["graph0_edges"]
    d_edges = torch.from_numpy(np.ascontiguousarray(e, np.float64)).cuda()
    vol = tree2img.voxelize_edges_device(d_edges, np.array([0, len(e)]), [1216, 1216, 16])[0]
    vol = (vol >= 1).to(torch.uint8).movedim(2, 0)[5:-4].contiguous().cpu().numpy()
    assert vol.shape == SHAPE, vol.shape
    return vol


def masks():
    rng = np.random.default_rng(0)
    field = (rng.random(SHAPE) < 0.08).astype(np.uint8)
    plane = field.copy()
    plane[SHAPE[0] // 2] = 1
    yield "(a) 8 % random field, plane filled", plane
    yield "(b) 8 % random field, no plane", field
    graph = np.maximum(fixture_volume(), (rng.random(SHAPE) < 0.02).astype(np.uint8))
    graph[SHAPE[0] // 2] = 1
    yield "(c) fixture graph + 2 % salt, plane filled", graph


def scipy_largest(mask):
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 3))
    counts = np.bincount(lab.ravel())
    best = int(np.argmax(counts[1:])) + 1 if n else 0
    return (lab == best) & (lab > 0), n, int(counts[best]) if n else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no_scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    torch.cuda.set_device(0)
    print(torch.cuda.get_device_name(0), flush=True)
    n = int(np.prod(SHAPE))
    for name, m in masks():
        d = torch.from_numpy(m).cuda()
        out, info = postprocess.cc3d_filter_device(d[None], 3, 1, return_info=True)
        info = info.cpu().numpy()[0]
        print(f"{name}: {int(np.count_nonzero(m))} foreground voxels ({np.count_nonzero(m) / n:.3%}), {info[0]} components, largest {info[1]}", flush=True)
        largest = small = slices = 0.0
        for _ in range(3):                                   # alternate the three
            largest += timed(lambda: postprocess.cc3d_filter_device(d[None], 3, 1), args.calls) / 3
            small += timed(lambda: postprocess.cc3d_filter_device(d[None], 3, 0, 16), args.calls) / 3
            slices += timed(lambda: postprocess.remove_small_objects_device(d, 16), args.calls) / 3
        for what, ms, mode in (("octa_cc3d_filter mode 1 (largest, 26)", largest, 1), ("octa_cc3d_filter mode 0 (min_size 16, 26)", small, 0)):
            b = hbm_bytes(m, 3, mode)
            print(f"  {what}: {ms:.3f} ms per call, {n / ms * 1e3:.3e} voxels/s; {b / 1e9:.2f} GB by count = {b / n:.1f} B/voxel, "
                  f"{b / (ms * 1e-3) / HBM_PEAK:.1%} of 8 TB/s", flush=True)
        print(f"  octa_remove_small_objects, B = 44 slices (min_size 16, 4-neighbourhood; the parent's per-slice filter): {slices:.3f} ms per call", flush=True)
        if not args.no_scipy:
            t0 = time.perf_counter()
            want, ncomp, size = scipy_largest(m)
            print(f"  scipy label + bincount + argmax, one CPU core, once: {time.perf_counter() - t0:.2f} s ({ncomp} components, largest {size})", flush=True)
            assert (ncomp, size) == (int(info[0]), int(info[1])) and np.array_equal(out[0].cpu().numpy() != 0, want)
            print("  the kernel's result equals scipy's", flush=True)


if __name__ == "__main__":
    main()
