"""Inference post-processing on the GPU: the `post_processing.prediction` list of the configs
(configs/config_ves_seg-S.yml:103-113: Activations(sigmoid) -> AsDiscrete(0.5) -> RemoveSmallObjects(160), label:
CastToType uint8) as used by test.py / validate.py, for a whole batch of logits in HBM."""
import torch

from .. import _native


def cc3d_filter_device(mask, connectivity, mode, min_size=0, on_value=1, return_info=False):
    """octa_cc3d_filter (csrc/cc3d.hip) on a CUDA mask [B,D,H,W] (non-zero = foreground): uint8 [B,D,H,W] with on_value on the voxels of
    the components kept -- mode 0: at least min_size voxels, mode 1: the largest of each volume, ties to the one whose first voxel comes
    first in C order. connectivity 1 / 2 / 3 = the 6- / 18- / 26-neighbourhood. return_info: also int64 [B,3] = number of components,
    voxels of the largest, flat index of its first voxel inside the volume (-1: no foreground)."""
    assert mask.is_cuda and mask.dim() == 4
    m = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()
    out = torch.empty_like(m)
    info = torch.empty((m.shape[0], 3), dtype=torch.int64, device=m.device) if return_info else None
    _native.launch("octa_cc3d_filter", m.device, m, m.shape[0], m.shape[1], m.shape[2], m.shape[3], int(connectivity), int(mode), int(min_size),
                   int(on_value), out, info)
    return (out, info) if return_info else out


def _as_volumes(mask):
    """[H,W] / [D,H,W] / [B,D,H,W] -> ([B,D,H,W] view, spatial rank)."""
    if mask.dim() == 2:
        return mask[None, None], 2
    if mask.dim() == 3:
        return mask[None], 3
    if mask.dim() == 4:
        return mask, 3
    raise ValueError(f"expected a mask [H,W], [D,H,W] or [B,D,H,W], got {tuple(mask.shape)}")


def keep_largest_component_device(mask, connectivity=None):
    """mask: CUDA [D,H,W], [B,D,H,W] or [H,W] (non-zero = foreground) -> uint8 0 / 1 of the same shape: the component with the most
    voxels of each volume (skimage.measure.label + argmax(bincount[1:]), what MONAI's KeepLargestConnectedComponent does for one
    label); a tie goes to the component whose first voxel comes first in C order. connectivity None = full for the rank (2-D: 2, 3-D: 3)."""
    assert mask.is_cuda
    vols, rank = _as_volumes(mask)
    connectivity = rank if connectivity is None else int(connectivity)
    if not 1 <= connectivity <= rank:
        raise ValueError(f"connectivity must be 1..{rank} for a {rank}-D mask, got {connectivity}")
    return cc3d_filter_device(vols, connectivity, 1).view(mask.shape)


def remove_small_objects_device(mask, min_size=64, connectivity=1, on_value=1, independent_channels=True):
    """mask: CUDA uint8 / bool [B,H,W] or [B,1,H,W] (non-zero = foreground) -> uint8 of the same shape with every
    connected component smaller than min_size removed (skimage.morphology.remove_small_objects semantics).
    independent_channels=False: the leading axis of a [C,H,W] mask is depth and the components are those of the volume
    (connectivity 1 / 2 / 3 = 6- / 18- / 26-neighbourhood, csrc/cc3d.hip)."""
    assert mask.is_cuda
    if not independent_channels:
        if mask.dim() != 3:
            raise ValueError(f"independent_channels=False expects a volume [C,H,W], got {tuple(mask.shape)}")
        return cc3d_filter_device(mask[None], connectivity, 0, min_size, on_value)[0]
    shape = mask.shape
    m = mask.reshape(-1, shape[-2], shape[-1]).to(torch.uint8).contiguous()
    out = torch.empty_like(m)
    _native.launch("octa_remove_small_objects", m.device, m, m.shape[0], m.shape[1], m.shape[2], int(min_size), int(connectivity), int(on_value), out)
    return out.view(shape)


def remove_outer_noise_device(volume, z_axis=0):
    """The reference's RemoveOuterNoise (data/data_transforms.py:418-432) on a CUDA volume [D,H,W]: everything not 26-connected to the
    central plane goes -- a boolean copy, plane `shape[z_axis] // 2` of DIM 0 filled (the reference indexes dim 0 whatever z_axis
    is; an index past dim 0 raises IndexError as there), the largest component of that, logical_and with the volume. torch.bool.
    The fill and the AND are two elementwise torch ops around the call."""
    if volume.dim() not in (2, 3):
        raise NotImplementedError(f"RemoveOuterNoise: the volume must have 2 or 3 dims, got {tuple(volume.shape)}")
    tmp = (volume != 0).to(torch.uint8)
    tmp[volume.shape[z_axis] // 2].fill_(1)
    return torch.logical_and(volume, keep_largest_component_device(tmp) != 0)


def postprocess_prediction(logits, post_config):
    """Apply the reference's `post_processing.prediction` list (names as in the YAML) to CUDA logits [B,1,H,W]."""
    x = logits
    for d in post_config:
        name = d["name"]
        if name == "Activations":
            if d.get("sigmoid", False):
                x = torch.sigmoid(x.float())
            elif d.get("softmax", False):
                x = torch.softmax(x.float(), dim=1)
        elif name == "AsDiscrete":
            if "threshold" in d:
                x = (x >= float(d["threshold"])).to(torch.uint8)
            elif d.get("argmax", False):
                x = x.argmax(dim=1, keepdim=True).to(torch.uint8)
        elif name == "RemoveSmallObjects":
            x = remove_small_objects_device(x, d.get("min_size", 64), d.get("connectivity", 1))
        elif name == "KeepLargestConnectedComponent":
            if x.shape[1] != 1:
                raise NotImplementedError("KeepLargestConnectedComponent: several channels are not supported")
            x = x * keep_largest_component_device(x, d.get("connectivity")).to(x.dtype)       # [B,1,H,W]: B volumes of depth 1
        elif name == "RemoveOuterNoise":                                                       # [B,C,H,W]: B volumes, the channels are depth
            tmp = (x != 0).to(torch.uint8)
            tmp[:, x.shape[1] // 2].fill_(1)
            x = torch.logical_and(x, keep_largest_component_device(tmp) != 0)
        elif name == "CastToType":
            x = x.to(torch.uint8)
        else:
            raise NotImplementedError(f"post-processing step {name} is not on the GPU path")
    return x
