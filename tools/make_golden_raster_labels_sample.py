"""tools/make_golden_raster_labels_sample.py -- generates tests/golden/raster_labels_sample_golden.npz.xz.

The reference ships 500 graph <-> label pairs (datasets/vessel_graphs/*.csv <-> datasets/labels/*.png).
tests/test_raster_oracle.py::test_oracle_reproduces_shipped_labels_sample checks every 100th pair of the sorted list. Two of those
five are already held by raster_golden.npz and raster_shipped_golden.npz (edge arrays and label bits; checked here); this fixture
holds the other three, exactly and compactly:

  * nodes in order of first appearance (a row's node2, then its node1); every coordinate as printed, i.e. an integer mantissa m and
    a decimal exponent x (value = m * 10**x, so float(f"{m}e{x}") is bit-identical to float() of the printed token). A node first seen
    as node1 of a row is stored as the difference to that row's node2 (its parent) taken at its own exponent:
    delta = m - floor(parent value / 10**x), parent value in exact units of 1e-16; other nodes (the roots) store m itself;
  * the rows' node indices, the distinct radii and the rows' radius indices;
  * the SHA-256 of the shipped label's pixels (PNG -> Pillow "L", uint8 {0, 255}, row-major).

The whole .npz is compressed with lzma (standard library), because the mantissas compress better as one stream.

  python tools/make_golden_raster_labels_sample.py <reference checkout>
"""
import csv
import hashlib
import io
import lzma
import os
import sys
from decimal import Decimal

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
OUT = os.path.join(GOLDEN, "raster_labels_sample_golden.npz.xz")


def tokens(s):
    return [c for c in s[1:-1].split(" ") if len(c) > 0]


def mantissa_exponent(t):
    d = Decimal(t).as_tuple()
    return int("".join(map(str, d.digits))) * (-1 if d.sign else 1), d.exponent


def encode(rows):
    ids, m, x, parent, ends = {}, [], [], [], []
    value = lambda nd: tuple(a * 10 ** (16 + b) for a, b in nd)          # exact, units of 1e-16: one node however it was printed
    for r in rows:
        n1 = tuple(mantissa_exponent(t) for t in tokens(r["node1"]))
        n2 = tuple(mantissa_exponent(t) for t in tokens(r["node2"]))
        for nd, par in ((n2, None), (n1, n2)):
            if value(nd) not in ids:
                ids[value(nd)] = len(m)
                m.append([a for a, _ in nd]); x.append([b for _, b in nd])
                parent.append(ids[value(par)] if par is not None else -1)
        ends.append((ids[value(n1)], ids[value(n2)]))
    m, x, parent = np.array(m, np.int64), np.array(x, np.int64), np.array(parent, np.int64)
    assert x.min() >= -16 and x.max() <= 0
    v = m * 10 ** (16 + x)
    delta = m.copy()
    has = parent >= 0
    delta[has] -= v[parent[has]] // 10 ** (16 + x[has])
    return delta, x.astype(np.int8), parent.astype(np.int32), np.array(ends, np.int32)


def decode(delta, x, parent, ends, radii, radius_index):
    """The inverse (tests/test_raster_oracle.py holds the same few lines): edge array [n, 7] in the CSV's row order."""
    v = [None] * len(delta)
    for k in range(len(delta)):
        v[k] = [(int(d) + (v[int(parent[k])][c] // 10 ** (16 + int(e)) if parent[k] >= 0 else 0)) * 10 ** (16 + int(e))
                for c, (d, e) in enumerate(zip(delta[k], x[k]))]
    nodes = np.array([[float(f"{a}e-16") for a in p] for p in v])
    return np.concatenate([nodes[ends[:, 0]], nodes[ends[:, 1]], radii[radius_index][:, None]], axis=1)


def main(ref):
    graphs, labels = os.path.join(ref, "datasets", "vessel_graphs"), os.path.join(ref, "datasets", "labels")
    names = [fn[:-4] for fn in sorted(os.listdir(graphs))[::100]]
    held = {str(np.load(os.path.join(GOLDEN, "raster_golden.npz"))["graph0_name"]): ("raster_golden.npz", "graph0_edges", "graph0_label_packed")}
    shipped = np.load(os.path.join(GOLDEN, "raster_shipped_golden.npz"))
    for k, n in enumerate(shipped["names"]):
        held[str(n)] = ("raster_shipped_golden.npz", f"edges_{k}", f"label_packed_{k}")
    g, new = {"names": np.array(names)}, []
    for name in names:
        with open(os.path.join(graphs, name + ".csv"), newline="") as fh:
            rows = list(csv.DictReader(fh))
        e = np.array([[float(c) for c in tokens(r["node1"]) + tokens(r["node2"])] + [float(r["radius"])] for r in rows])
        lab = np.array(Image.open(os.path.join(labels, name + ".png")).convert("L"))
        if name in held:                          # the fixture that holds it must hold exactly this pair
            f, ek, lk = held[name]
            h = np.load(os.path.join(GOLDEN, f))
            assert h[ek].shape == e.shape and (h[ek] == e).all(), name
            assert (np.unpackbits(h[lk])[: lab.size].reshape(lab.shape) * 255 == lab).all(), name
            continue
        k = len(new)
        delta, x, parent, ends = encode(rows)
        radii, radius_index = np.unique(e[:, 6], return_inverse=True)
        assert (decode(delta, x, parent, ends, radii, radius_index) == e).all(), name
        g.update({f"delta_{k}": delta, f"exp_{k}": x, f"parent_{k}": parent, f"ends_{k}": ends, f"radii_{k}": radii,
                  f"radius_index_{k}": radius_index.astype(np.int32),
                  f"label_sha256_{k}": np.array(hashlib.sha256(np.ascontiguousarray(lab, np.uint8).tobytes()).hexdigest())})
        new.append(name)
    g["new_names"] = np.array(new)
    buf = io.BytesIO()
    np.savez(buf, **g)
    with open(OUT, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print("wrote", os.path.abspath(OUT), os.path.getsize(OUT) // 1024, "KiB;", "stored:", new, "held elsewhere:", sorted(set(names) - set(new)))


if __name__ == "__main__":
    main(sys.argv[1])
