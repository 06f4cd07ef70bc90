"""Adversarial augmentation (reference utils/losses.py:11-109 ANTLoss with models/noise_model.py NoiseModel.forward(adversarial=True); the
set-up of configs/config_ves_seg-S_AA.yml): the noise model's five control grids are moved three gradient steps UP the segmentation loss of
the frozen network, and the sample drawn from the moved grids is what the network then trains on.

Per call, in the reference's order:
  * python `random` (the global stream as in the reference, or with `seed` a private random.Random, which is what LambdaModel asks for: the
    device loader's thread advances the global stream at its own pace): downsample_factor per sample (uniform(max_decrease_res, 1)); the crop offsets per sample (randint, rows then columns)
    if crop != (1, 1); rot_k per sample (choice of 0..3); rot_r per sample (uniform(-10, 10) degrees);
  * label: rot90 + bilinear rotation, crop, threshold at label_threshold;
  * torch's global generator: the control grids (data/noise_model.py NoiseModelDraws: the first call of an instance draws them twice);
  * sample = crop(rotate(nearest down / up(bilinear resize to the label's size(noise model(image, background, grids)))));
  * three times: loss of the frozen network on the sample, backward of -loss * grad_scale, grids += -alpha * grids.grad (the reference's SGD step
    on the gradient of scaler.scale(-loss), which it never unscales), a new sample from the moved grids. The last one is made without a graph
    and returned detached with the cropped label.

Device tensors ([B, 1, H, W]; image, background and label are taken to float32 first, so the label comes back in float32) take the noise model and its backward from csrc/noise_model.hip (data/gpu_augment.py
noise_model_rsample: per-pixel Beta fields from a counter-based generator, one fresh 64-bit seed per sample draw from torch's generator;
the backward redraws them) and the bilinear resize from csrc/augment.hip; the nearest resamples, the rotation and the crop are torch ops that
autograd differentiates. Host tensors take the torch restatement (data/noise_model.py noise_model_host with Beta.rsample), which is the
reference's arithmetic: tests/test_noise_model_at.py holds it against recorded runs of the reference's own classes.

grad_scale: the reference's step is alpha x the GradScaler's scale, 65536 when training starts and drifting with the scaler afterwards. This
package trains in bf16 without loss scaling, so the factor is a setting, `Train.AT.grad_scale`, default 65536.0; the drift is not reproduced.

The rotation restates torchvision.transforms.functional.rotate(img, angle, BILINEAR) (inverse affine matrix of -angle about the centre, its
base grid, grid_sample with zeros padding, align_corners False). torchvision is not installed where this was written: parity with
torchvision itself is unpinned."""
import math
import random

import torch
import torch.nn.functional as F

from ..data.noise_model import NoiseModelDraws, noise_model_host

NUM_ITERS = 3


def rotate_bilinear(img: torch.Tensor, angle: float) -> torch.Tensor:
    """torchvision.transforms.functional.rotate(img, angle, InterpolationMode.BILINEAR) for a float tensor [N, C, H, W]: counter-clockwise by
    `angle` degrees about the centre, same size, zeros outside."""
    rot = math.radians(-angle)
    # _get_inverse_affine_matrix(center (0, 0), -angle, no translation, scale 1, no shear)
    matrix = [math.cos(rot), math.sin(rot), 0.0, -math.sin(rot), math.cos(rot), 0.0]
    h, w = img.shape[-2:]
    theta = torch.tensor(matrix, dtype=img.dtype, device=img.device).reshape(1, 2, 3)
    base = torch.empty(1, h, w, 3, dtype=img.dtype, device=img.device)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w, device=img.device))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h, device=img.device).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=img.dtype, device=img.device)
    grid = base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2).expand(img.shape[0], h, w, 2)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


class AtLoss:
    """get_loss_function_by_name("AtLoss", config, scaler, loss): called as at(model, image, background, label) -> (adversarial image, label)."""

    def __init__(self, loss_fun, grid_size=(9, 9), lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, max_decrease_res=0.25, alpha=1e-3,
                 crop=(1, 1), label_threshold=0.1, grad_scale=65536.0, autocast=None, rotate=rotate_bilinear, seed=None):
        self.loss_fun = loss_fun
        self.draws = NoiseModelDraws(tuple(grid_size))
        self.lambdas = (lambda_delta, lambda_speckle, lambda_gamma)
        self.max_decrease_res = max_decrease_res
        self.alpha = alpha
        self.crop = tuple(crop)
        self.label_threshold = label_threshold
        self.grad_scale = float(grad_scale)
        self.autocast = autocast          # a context-manager factory (BaseModelABC.autocast); None: run as called
        self.rotate = rotate
        # the geometry draws. seed None: the global `random`, as the reference. An integer: a private stream -- the device loader prepares its
        # batches from a thread of its own and advances the global `random` there (LoadGraphAndFilterByRandomRadiusd), so draws made from the
        # training thread would interleave with it by timing; LambdaModel passes General.seed
        self.rng = random if seed is None else random.Random(int(seed))
        self.grids = None                 # [B, 5, gh, gw] of the last call, after its steps
        self.grid_trajectory = []         # the grids as drawn and after each step (detached copies)
        self.loss_trajectory = []         # the three losses (0-dim tensors; reading one synchronises)

    # ---- the call's random geometry --------------------------------------------------------------------------------------------------
    def _randomize(self, x, y):
        n = x.shape[0]
        self.downsample_factor = [self.rng.uniform(self.max_decrease_res, 1) for _ in range(n)]
        if self.crop != (1, 1):
            self.len_h, self.len_w = int(y.shape[-2] * self.crop[0]), int(y.shape[-1] * self.crop[1])
            self.h_crop = [self.rng.randint(0, y.shape[-2] - self.len_h) for _ in range(n)]
            self.w_crop = [self.rng.randint(0, y.shape[-1] - self.len_w) for _ in range(n)]
        self.rot_k = [self.rng.choice([0, 1, 2, 3]) for _ in range(n)]
        self.rot_r = [self.rng.uniform(-10, 10) for _ in range(n)]

    def _crop_sample(self, t):
        if self.crop == (1, 1):
            return t
        return torch.stack([t[b, :, self.h_crop[b]:self.h_crop[b] + self.len_h, self.w_crop[b]:self.w_crop[b] + self.len_w] for b in range(t.shape[0])], dim=0)

    def _rand_decrease_res(self, img):
        out = []
        for b in range(img.shape[0]):
            tmp = F.interpolate(img[b:b + 1], scale_factor=self.downsample_factor[b])
            out.append(F.interpolate(tmp, size=img.shape[-2:])[0])
        return torch.stack(out, dim=0)

    def _rand_rotate(self, img):
        return torch.stack([self.rotate(torch.rot90(img[b:b + 1], self.rot_k[b], dims=(-2, -1)), self.rot_r[b])[0] for b in range(img.shape[0])], dim=0)

    # ---- the sample of the current grids -----------------------------------------------------------------------------------------------
    def _noise_model(self, x, background, grids):
        if not x.is_cuda:
            return noise_model_host(x, background, [grids[:, k:k + 1] for k in range(5)], *self.lambdas)
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32 or background.shape != x.shape or background.dtype != torch.float32:
            raise ValueError(f"AtLoss on the device takes float32 [B, 1, H, W] images and backgrounds of one shape (csrc/noise_model.hip); got "
                             f"{tuple(x.shape)} {x.dtype} and {tuple(background.shape)} {background.dtype}")
        from ..data.gpu_augment import noise_model_rsample
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        return noise_model_rsample(x[:, 0], background[:, 0], grids, seed, *self.lambdas).unsqueeze(1)

    def _resize(self, s, size):
        if s.is_cuda:
            from ..data.gpu_augment import BilinearResize
            return BilinearResize.apply(s, tuple(int(v) for v in size))
        return F.interpolate(s, size=size, mode="bilinear")

    def _sample(self, x, background, y, grids):
        s = self._noise_model(x, background, grids)
        s = self._resize(s, y.shape[-2:])
        s = self._rand_decrease_res(s)
        s = self._rand_rotate(s)
        return self._crop_sample(s)

    def _forward_loss(self, model, sample, y_crop):
        pred = model(sample)
        return self.loss_fun(pred.float(), y_crop.float())

    def __call__(self, model, x, background, y):
        if x.is_cuda:
            # the loader's CastToTyped hands image and label over in the training dtype (bf16 under General.amp). The noise model's arithmetic is
            # float32, and so is the rotation's sampling grid: in bf16 the pixel coordinates of a 1216^2 label have a quantum of 2 - 4 pixels
            x, background, y = x.float(), background.float(), y.float()
        flags = [(p, p.requires_grad) for p in model.parameters()]
        model.requires_grad_(False)
        try:
            with torch.no_grad():
                self._randomize(x, y)
                y = self._rand_rotate(y)
                y_crop = self._crop_sample(y).clone()
                y_crop[y_crop < self.label_threshold] = 0.
                y_crop[y_crop >= self.label_threshold] = 1.
            with torch.no_grad():
                # as the reference's parameters, the grids keep the batch size of the instance's first call; a smaller batch uses the first rows
                grids = torch.cat(self.draws.control_points(x.shape[0], x.dtype), dim=1)[:x.shape[0]].contiguous().to(x.device)
            grids.requires_grad_(True)
            self.grid_trajectory, self.loss_trajectory = [grids.detach().clone()], []
            with torch.enable_grad():
                adv = self._sample(x, background, y, grids)
            for i in range(NUM_ITERS):
                with torch.enable_grad():
                    if self.autocast is not None:
                        with self.autocast():
                            loss = self._forward_loss(model, adv, y_crop)
                    else:
                        loss = self._forward_loss(model, adv, y_crop)
                    self.loss_trajectory.append(loss.detach())
                    grids.grad = None
                    (-loss * self.grad_scale).backward()
                with torch.no_grad():
                    grids.add_(grids.grad, alpha=-self.alpha)          # SGD on -loss: ascent on the loss
                self.grid_trajectory.append(grids.detach().clone())
                with torch.set_grad_enabled(i < NUM_ITERS - 1):
                    adv = self._sample(x, background, y, grids)
            self.grids = grids.detach()
        finally:
            for p, flag in flags:
                p.requires_grad_(flag)
        return adv.detach(), y_crop
