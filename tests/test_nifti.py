"""CPU: the NIfTI-1 single-file reader / writer (octa_autosegmentation_amd/nifti.py) against the format's standard header offsets."""
import gzip
import struct

import numpy as np
import pytest

from octa_autosegmentation_amd import nifti

DTYPES = {"uint8": (2, 8), "int16": (4, 16), "uint16": (512, 16), "int32": (8, 32), "float32": (16, 32), "float64": (64, 64)}
SHAPES = [(3, 4, 5), (7, 1, 2, 3), (1, 1, 1)]


def _array(shape, dtype, seed=0):
    r = np.random.RandomState(seed)
    if np.dtype(dtype).kind == "f":
        return r.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    return r.randint(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


def _raw(path):
    return gzip.open(path, "rb").read() if str(path).endswith(".gz") else open(path, "rb").read()


@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_round_trip_and_header(tmp_path, dtype, shape, ext):
    a = _array(shape, dtype, seed=len(shape))
    affine = np.array([[2.0, 0, 0, -7], [0, 0.5, 0, 3], [0.25, 0, 1, 11], [0, 0, 0, 1]])
    path = str(tmp_path / ("v" + ext))
    nifti.write(path, a, affine)
    got, hdr = nifti.read(path)
    assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a)
    assert np.array_equal(hdr["affine"], affine) and hdr["sform_code"] == 2 and hdr["byteorder"] == "<"
    raw = _raw(path)
    assert (open(path, "rb").read(2) == b"\x1f\x8b") == ext.endswith(".gz")
    assert struct.unpack_from("<i", raw, 0)[0] == 348                                          # sizeof_hdr
    dim = struct.unpack_from("<8h", raw, 40)
    assert dim[0] == len(shape) and dim[1:1 + len(shape)] == shape and all(d == 1 for d in dim[1 + len(shape):])
    assert struct.unpack_from("<hh", raw, 70) == DTYPES[dtype]                                 # datatype, bitpix
    assert struct.unpack_from("<8f", raw, 76) == (1.0,) * 8                                    # pixdim
    assert struct.unpack_from("<f", raw, 108)[0] == 352.0                                      # vox_offset
    assert struct.unpack_from("<h", raw, 254)[0] == 2                                          # sform_code
    assert struct.unpack_from("<4f", raw, 280) == tuple(affine[0])                             # srow_x
    assert struct.unpack_from("<4f", raw, 296) == tuple(affine[1]) and struct.unpack_from("<4f", raw, 312) == tuple(affine[2])
    assert raw[344:348] == b"n+1\0" and raw[348:352] == b"\0\0\0\0"
    assert raw[352:] == a.tobytes(order="F")                                                   # x fastest


def test_default_affine_is_the_identity(tmp_path):
    path = str(tmp_path / "v.nii")
    nifti.write(path, np.zeros((2, 3, 4), np.uint8))
    assert np.array_equal(nifti.read(path)[1]["affine"], np.eye(4))


def _big_endian_file(shape, values, slope, inter, datatype=4, bitpix=16, fmt=">i2"):
    hdr = bytearray(348)
    struct.pack_into(">i", hdr, 0, 348)
    struct.pack_into(">8h", hdr, 40, len(shape), *(list(shape) + [1] * (7 - len(shape))))
    struct.pack_into(">hh", hdr, 70, datatype, bitpix)
    struct.pack_into(">8f", hdr, 76, *([1.0] * 8))
    struct.pack_into(">f", hdr, 108, 352.0)
    struct.pack_into(">ff", hdr, 112, slope, inter)
    struct.pack_into(">hh", hdr, 252, 0, 2)
    for k in range(3):
        struct.pack_into(">4f", hdr, 280 + 16 * k, *np.eye(4)[k])
    hdr[344:348] = b"n+1\0"
    return bytes(hdr) + b"\0\0\0\0" + np.asarray(values).astype(fmt).tobytes(order="F")


def test_big_endian_file_with_scaling(tmp_path):
    a = np.arange(-12, 12, dtype=np.int16).reshape(2, 3, 4)
    for ext, opener in ((".nii", open), (".nii.gz", gzip.open)):
        path = str(tmp_path / ("be" + ext))
        with opener(path, "wb") as f:
            f.write(_big_endian_file(a.shape, a, 2.0, 1.0))
        got, hdr = nifti.read(path)
        assert hdr["byteorder"] == ">" and hdr["scl_slope"] == 2.0 and hdr["scl_inter"] == 1.0
        assert got.dtype == np.float64 and np.array_equal(got, a.astype(np.float64) * 2.0 + 1.0)
    # slope 0 and NaN: the stored values, in the stored dtype
    for slope in (0.0, float("nan")):
        path = str(tmp_path / "raw.nii")
        with open(path, "wb") as f:
            f.write(_big_endian_file(a.shape, a, slope, 5.0))
        got, _ = nifti.read(path)
        assert got.dtype == np.int16 and np.array_equal(got, a)


def test_bad_files_are_refused_with_a_message(tmp_path):
    a = _array((3, 4, 5), "int16")
    good = str(tmp_path / "good.nii")
    nifti.write(good, a)
    raw = open(good, "rb").read()

    def refuse(name, blob, match, opener=open):
        path = str(tmp_path / name)
        with opener(path, "wb") as f:
            f.write(blob)
        with pytest.raises(nifti.NiftiError, match=match):
            nifti.read(path)

    refuse("short_header.nii", raw[:100], "shorter than the 348-byte")
    refuse("short_data.nii", raw[:-1], "truncated")
    refuse("short_data.nii.gz", raw[:-7], "truncated", gzip.open)
    gz = str(tmp_path / "full.nii.gz")
    nifti.write(gz, a)
    refuse("cut.nii.gz", open(gz, "rb").read()[:60], "not a readable NIfTI-1 file")
    for code in (0, 1, 32, 128, 256, 768, 1024, 2304):           # none, binary, complex64, rgb24, int8, uint32, int64, rgba32
        blob = bytearray(raw)
        struct.pack_into("<h", blob, 70, code)
        refuse("dt.nii", bytes(blob), "datatype code %d is not supported" % code)
    blob = bytearray(raw)
    blob[344:348] = b"ni1\0"
    refuse("pair.nii", bytes(blob), "only single-file")
    blob = bytearray(raw)
    struct.pack_into("<i", blob, 0, 540)
    refuse("nifti2.nii", bytes(blob), "sizeof_hdr is not 348")
    with pytest.raises(nifti.NiftiError, match="dtype"):
        nifti.write(str(tmp_path / "x.nii"), np.zeros((2, 2), np.int64))
    with pytest.raises(nifti.NiftiError, match="dimensions"):
        nifti.write(str(tmp_path / "x.nii"), np.zeros((1, 1, 1, 1, 1), np.uint8))
