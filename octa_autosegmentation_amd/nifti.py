"""NIfTI-1 single-file volumes (`.nii`, `.nii.gz`) without nibabel: a 348-byte header, four extension bytes and the raw array, x
fastest. Written from the NIfTI-1 specification (nifti1.h); what `nib.save(nib.Nifti1Image(array, affine), path)` and
`nib.load(path).get_fdata()` are used for in the reference (label volumes of the 3-D reconstruction set-up, 3-D predictions).
nibabel is absent here, so parity with its files is unpinned: the tests pin the header fields at their standard offsets."""
import gzip
import struct
import zlib

import numpy as np

# numpy dtype -> (datatype code, bitpix)
_CODES = {np.dtype(np.uint8): (2, 8), np.dtype(np.int16): (4, 16), np.dtype(np.int32): (8, 32), np.dtype(np.float32): (16, 32),
          np.dtype(np.float64): (64, 64), np.dtype(np.uint16): (512, 16)}
_DTYPES = {code: dt for dt, (code, _) in _CODES.items()}
HEADER_BYTES, VOX_OFFSET = 348, 352


class NiftiError(ValueError):
    pass


def _is_gz(path):
    return str(path).endswith(".gz")


def write(path, array, affine=None):
    """`array` (1 to 4 dims; uint8, int16, uint16, int32, float32 or float64) -> `path` (.nii or .nii.gz). Header: sizeof_hdr 348, dim,
    datatype / bitpix, pixdim 1, vox_offset 352, no intensity scaling, qform_code 0, sform_code 2 with `affine` (4x4, default identity) in
    srow_x/y/z, magic `n+1`; then four zero extension bytes and the voxels in Fortran order, little-endian."""
    a = np.asarray(array)
    if a.dtype.newbyteorder("=") not in _CODES:
        raise NiftiError(f"nifti.write: dtype {a.dtype} is not supported (uint8, int16, uint16, int32, float32, float64)")
    if not 1 <= a.ndim <= 4:
        raise NiftiError(f"nifti.write: {a.ndim} dimensions (1 to 4 are supported)")
    if any(s < 1 or s > 32767 for s in a.shape):
        raise NiftiError(f"nifti.write: shape {a.shape} does not fit the header's int16 dim[]")
    aff = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    if aff.shape != (4, 4):
        raise NiftiError("nifti.write: the affine must be 4 x 4")
    code, bitpix = _CODES[a.dtype.newbyteorder("=")]
    hdr = bytearray(HEADER_BYTES)
    struct.pack_into("<i", hdr, 0, HEADER_BYTES)                                    # sizeof_hdr
    hdr[38] = ord("r")                                                              # regular
    struct.pack_into("<8h", hdr, 40, a.ndim, *(list(a.shape) + [1] * (7 - a.ndim)))  # dim
    struct.pack_into("<hh", hdr, 70, code, bitpix)                                  # datatype, bitpix
    struct.pack_into("<8f", hdr, 76, 1, 1, 1, 1, 1, 1, 1, 1)                        # pixdim (qfac = 1)
    struct.pack_into("<f", hdr, 108, float(VOX_OFFSET))                             # vox_offset
    struct.pack_into("<ff", hdr, 112, float("nan"), float("nan"))                   # scl_slope / scl_inter: not set
    struct.pack_into("<hh", hdr, 252, 0, 2)                                         # qform_code = unknown, sform_code = aligned
    for k in range(3):
        struct.pack_into("<4f", hdr, 280 + 16 * k, *aff[k])                         # srow_x, srow_y, srow_z
    hdr[344:348] = b"n+1\0"
    payload = bytes(hdr) + b"\0\0\0\0" + a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes(order="F")
    if _is_gz(path):
        with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(payload)
    else:
        with open(path, "wb") as f:
            f.write(payload)
    return path


def read(path):
    """-> (array, header). The array has the stored axis order and dtype (native byte order); when scl_slope is neither 0 nor NaN it is
    float64 `stored * scl_slope + scl_inter`. header: dict of dim, datatype, bitpix, pixdim, vox_offset, scl_slope, scl_inter,
    qform_code, sform_code, affine (the srow rows as a 4 x 4 float64), byteorder ('<' or '>'). Either byte order is read and extensions
    in front of a later vox_offset are skipped; two-file volumes, other datatypes and more than 4 dims are refused."""
    with (gzip.open(path, "rb") if _is_gz(path) else open(path, "rb")) as f:
        try:
            blob = f.read()
        except (OSError, EOFError, zlib.error) as e:
            raise NiftiError(f"{path}: not a readable NIfTI-1 file ({e})") from None
    if len(blob) < HEADER_BYTES:
        raise NiftiError(f"{path}: {len(blob)} bytes, shorter than the 348-byte NIfTI-1 header")
    order = None
    for o in "<>":
        if struct.unpack_from(o + "i", blob, 0)[0] == HEADER_BYTES:
            order = o
    if order is None:
        raise NiftiError(f"{path}: sizeof_hdr is not 348 in either byte order: not a NIfTI-1 file")
    magic = bytes(blob[344:348])
    if magic != b"n+1\0":
        raise NiftiError(f"{path}: magic {magic!r}: only single-file NIfTI-1 ('n+1') is supported")
    dim = struct.unpack_from(order + "8h", blob, 40)
    if not 1 <= dim[0] <= 7 or any(d < 1 for d in dim[1:dim[0] + 1]):
        raise NiftiError(f"{path}: bad dim {dim}")
    shape = list(dim[1:dim[0] + 1])
    while len(shape) > 4 and shape[-1] == 1:                          # trailing singleton axes beyond the fourth carry nothing
        shape.pop()
    if len(shape) > 4:
        raise NiftiError(f"{path}: {len(shape)} dimensions {tuple(shape)} (up to 4 are supported)")
    datatype, bitpix = struct.unpack_from(order + "hh", blob, 70)
    if datatype not in _DTYPES:
        raise NiftiError(f"{path}: datatype code {datatype} is not supported (2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, 512 uint16)")
    dt = _DTYPES[datatype]
    if bitpix != dt.itemsize * 8:
        raise NiftiError(f"{path}: bitpix {bitpix} does not match datatype code {datatype}")
    pixdim = struct.unpack_from(order + "8f", blob, 76)
    vox_offset, slope, inter = struct.unpack_from(order + "3f", blob, 108)
    if not vox_offset >= VOX_OFFSET or vox_offset != int(vox_offset):
        raise NiftiError(f"{path}: vox_offset {vox_offset} (a single-file volume starts at byte 352 or later)")
    qform_code, sform_code = struct.unpack_from(order + "hh", blob, 252)
    affine = np.eye(4)
    for k in range(3):
        affine[k] = struct.unpack_from(order + "4f", blob, 280 + 16 * k)
    count = int(np.prod(shape, dtype=np.int64))
    start, need = int(vox_offset), count * dt.itemsize
    if len(blob) < start + need:
        raise NiftiError(f"{path}: truncated: {len(blob) - start} data bytes, shape {tuple(shape)} {dt} needs {need}")
    a = np.frombuffer(blob, dtype=dt.newbyteorder(order), count=count, offset=start).reshape(shape, order="F")
    a = a.astype(dt)                                                  # native byte order, own memory
    if slope != 0 and not np.isnan(slope):
        a = a.astype(np.float64) * float(slope) + (0.0 if np.isnan(inter) else float(inter))
    header = {"dim": tuple(dim), "datatype": datatype, "bitpix": bitpix, "pixdim": tuple(pixdim), "vox_offset": float(vox_offset),
              "scl_slope": float(slope), "scl_inter": float(inter), "qform_code": qform_code, "sform_code": sform_code, "affine": affine,
              "byteorder": order}
    return a, header
