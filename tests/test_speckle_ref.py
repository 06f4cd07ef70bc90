"""Proves tests/_speckle_ref.py without a GPU: an fp32 emulation of the speckle passes of csrc/augment.hip (the control grid through the
resize emulation of tests/test_resize_ref.py, R and v with one rounding per operation, the extrema through the kernel's order-preserving
integer map on the floats' bit patterns, the two quotients and their difference) stays inside the bound on every case that
tests/test_speckle_gpu.py runs, meets the exact claims, and each wrong kernel (a mutant of the emulation) breaks the bound. Subtracting
the minimum before dividing is the same in exact arithmetic and has to pass: the bound is no artefact of the order of operations."""
import pytest
import torch

import _speckle_ref as S
from test_resize_ref import emulate_forward


def f2ord(v, fixup=True):
    i = v.contiguous().view(torch.int32)
    return torch.where(i >= 0, i, i ^ 0x7FFFFFFF) if fixup else i


def ord2f(i, fixup=True):
    return (torch.where(i >= 0, i, i ^ 0x7FFFFFFF) if fixup else i).contiguous().view(torch.float32)


def emulate(img, grid9, u, mut=None):
    B, H, W = img.shape
    C = emulate_forward(grid9, H, W, mut="align_corners" if mut == "align_corners" else None)
    R = C - u * (1.0 - C)
    v = img * R
    fix = mut != "no_sign_fixup"
    o = f2ord(v, fix).reshape(B, -1)
    omx, omn = o.amax(1), o.amin(1)
    if mut == "shared_minmax":
        omx, omn = omx.max().expand(B), omn.min().expand(B)
    mx, mn = ord2f(omx, fix)[:, None, None], ord2f(omn, fix)[:, None, None]
    if mut == "min_first":
        return (v - mn) / mx
    return v / mx - mn / mx


IDS = lambda s: "x".join(map(str, s))


def test_the_order_map_orders_floats():
    v = torch.tensor([float("-inf"), -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, float("inf")])
    o = f2ord(v)
    assert bool((o[1:] > o[:-1]).all()) and torch.equal(ord2f(o).view(torch.int32), v.view(torch.int32))
    assert not bool((f2ord(v, False)[1:] > f2ord(v, False)[:-1]).all())


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_emulation_is_within_the_bound_and_exact_where_claimed(shape):
    rat = {}
    for name, img, grid9, u in S.cases(shape):
        ref, tol = S.reference(img, grid9, u)
        assert float(ref.amin((1, 2)).abs().max()) == 0.0
        got = emulate(img, grid9, u)
        rat[name] = S.ratio(got, ref, tol)
        rat[name + ", minimum first"] = S.ratio(emulate(img, grid9, u, "min_first"), ref, tol)
        assert not bool(torch.isnan(got).any())
        assert torch.equal(got.amin((1, 2)), torch.zeros(shape[0])), name
        if name == "negative":
            assert float((img * 1.0).amin()) < 0 and float(ref.amax()) > 1.0          # a negative minimum: the output passes 1
    print("RATIO", shape, {k: float(f"{v:.3g}") for k, v in rat.items()})
    assert all(v <= 1.0 for v in rat.values()), rat


MUTANTS = ("no_sign_fixup", "shared_minmax", "align_corners")


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_rejected(mut):
    caught = []
    for shape in S.SHAPES:
        for name, img, grid9, u in S.cases(shape):
            if not S.ratio(emulate(img, grid9, u, mut), *S.reference(img, grid9, u)) <= 1.0:
                caught.append(f"{IDS(shape)} {name}")
    print("MUTANT", mut, "caught on", caught)
    assert caught, f"no bound notices the mutant {mut}"
    if mut == "no_sign_fixup":
        assert all(c.endswith("negative") for c in caught) and len(caught) == 4
    if mut == "shared_minmax":
        assert sum(c.endswith("isolation") for c in caught) == 4
