"""CycleGAN, the paper's unpaired-translation baseline (reference models/cycle_gan.py:11-336, config
configs/experiment_configs/config_cycle_gan.yml): generators G_A (synthetic -> real contrast) and G_B (back), PatchGANs D_A (judges
G_A's images against real_B) and D_B (judges G_B's against real_A), two Adam optimisers (G_A + G_B, D_A + D_B; betas (0.5, 0.999)).
Per step (cycle_gan.py:169-228):

  background  bg = batch["background"] (or rand_like(real_A)) * uniform(0, 1)             -- torch's global generator, in this order
  forward     fake_B = G_A(max(real_A, bg)); rec_A = G_B(fake_B); fake_A = G_B(real_B); rec_B = G_A(max(fake_A, bg));
              with lambda_idt > 0: idt_A = G_A(real_B), idt_B = G_B(real_A)
  G update    D_A, D_B frozen:  loss_G = LSGAN(D_A(fake_B), 1) + LSGAN(D_B(fake_A), 1) + lambda_A L1(rec_A, real_A) + lambda_B L1(rec_B, real_B)
                                         + lambda_B lambda_idt L1(idt_A, real_B) + lambda_A lambda_idt L1(idt_B, real_A)
  D update    loss_D_A = (LSGAN(D_A(real_B), 1) + LSGAN(D_A(pool_B(fake_B)), 0)) / 2, loss_D_B likewise with real_A (the raw one) and
              pool_A(fake_A); pool_B is queried before pool_A; two backward passes, one optimiser step.

`lambda_idt = 0`: the reference fails there (`.item()` on the integer 0, cycle_gan.py:194-195, 245-246); here the two identity passes are
skipped, the `idt_A` / `idt_B` losses are reported as 0 and the `idt_A` output is None.

MI355X formulation, under bf16 autocast: passes that share weights run as ONE launch sequence over the concatenated batch --
G_A(max(real_A, bg) | real_B) = fake_B | idt_A, G_B(fake_B | real_B | real_A) = rec_A | fake_A | idt_B, G_A(max(fake_A, bg)) = rec_B,
D_A(real_B | pooled fake_B), D_B(real_A | pooled fake_A): three generator sequences instead of six, two discriminator sequences
instead of four in the D update. Every network normalises per sample (InstanceNorm), so each slice is what its own pass gives (CPU
tensors run the reference's own sequence of passes: USE_BATCHED_PASSES below). The
elementwise tail (mixing, L1 and LSGAN terms, the pools) runs on csrc/gan_loss.hip (models/gan_loss.py). Everything is queued on the
current stream.

ImagePool keeps the reference's draws (Python's global `random`, image by image) on the host and the images in one device tensor."""
import random
from typing import Any, Callable, Dict, Tuple

import torch
from torch import nn

from ..utils.enums import Phase
from . import gan_loss
from .base_model_abc import BaseModelABC, LossValues
from .lambda_model import decollate_batch
from .losses import LSGANLoss, get_loss_function_by_name
from .model_interface_abc import Output


# Passes that share weights as one launch sequence over the concatenated batch. None: for CUDA tensors only. On the CPU the reference's own
# sequence of passes runs instead: there the batched form changes the convolutions' summation order, three Adam steps amplify that to
# 1e-2 in the fourth step's gradient norms, while the unbatched step reproduces the reference's gradients bit for bit
# (tests/test_cycle_gan.py). True / False force either form on any device.
USE_BATCHED_PASSES = None


class ImagePool:
    """History of generated images (reference models/cycle_gan.py:287-336). While fewer than `pool_size` images are stored, an image is
    stored and returned; afterwards p = random.uniform(0, 1) is drawn per image and only for p > 0.5 a slot random.randint(0, pool_size - 1):
    the slot's image is returned and the current one takes its place. `pool_size = 0` returns the input.

    The images live in ONE tensor [pool_size, C, H, W] of the first query's dtype and device. A query makes the draws in the reference's
    order and resolves them into two tables -- per returned image its source (an input, or the OLD content of a slot), per touched slot
    the input that ends up in it -- which one launch applies (gan_loss.pool_exchange_device; CPU tensors: gan_loss.pool_exchange_host).
    Two images of one batch that draw the same slot: the second receives the first, the slot keeps the second."""

    def __init__(self, pool_size: int):
        self.pool_size = int(pool_size)
        self.num_imgs = 0
        self.images: torch.Tensor = None

    def resolve(self, batch: int):
        """The draws of one query of `batch` images -> (src, wslot, winput); src[b] = k >= 0: input k, -1 - s: old content of slot s."""
        now = {}                                    # slot -> the input that sits in it so far
        src = []
        for k in range(batch):
            if self.num_imgs < self.pool_size:
                now[self.num_imgs] = k
                self.num_imgs += 1
                src.append(k)
            elif random.uniform(0, 1) > 0.5:
                s = random.randint(0, self.pool_size - 1)
                src.append(now[s] if s in now else -1 - s)
                now[s] = k
            else:
                src.append(k)
        return src, list(now.keys()), list(now.values())

    def query(self, images: torch.Tensor) -> torch.Tensor:
        if self.pool_size == 0:
            return images
        images = images.detach().contiguous()
        if self.images is None:
            self.images = torch.zeros((self.pool_size,) + tuple(images.shape[1:]), dtype=images.dtype, device=images.device)
        if images.shape[1:] != self.images.shape[1:] or images.dtype != self.images.dtype or images.device != self.images.device:
            raise ValueError(f"ImagePool holds {tuple(self.images.shape[1:])} {self.images.dtype} images on {self.images.device}; got "
                             f"{tuple(images.shape[1:])} {images.dtype} on {images.device}")
        on_kernels = images.is_cuda and gan_loss.USE_FUSED_GAN_LOSS
        out = []
        for lo in range(0, images.shape[0], gan_loss.POOL_MAX_BATCH):       # one launch takes up to 32 images
            part = images[lo:lo + gan_loss.POOL_MAX_BATCH]
            tables = self.resolve(part.shape[0])
            out.append((gan_loss.pool_exchange_device if on_kernels else gan_loss.pool_exchange_host)(self.images, part, *tables))
        return out[0] if len(out) == 1 else torch.cat(out)


class CycleGAN(BaseModelABC):
    def __init__(self, phase: Phase, MODEL_DICT: dict, inference: str, netG_A_config: dict, netG_B_config: dict, netD_A_config: dict,
                 netD_B_config: dict, lambda_A: float, lambda_B: float, lambda_idt: float, pool_size: int, *args, **kwargs) -> None:
        super().__init__(optimizer_mapping={"optimizer_G": ["netG_A", "netG_B"], "optimizer_D": ["netD_A", "netD_B"]}, *args, **kwargs)
        self.lambda_A, self.lambda_B, self.lambda_idt = float(lambda_A), float(lambda_B), float(lambda_idt)
        self.netG_A: nn.Module = None
        self.netG_B: nn.Module = None
        self.netD_A: nn.Module = None
        self.netD_B: nn.Module = None
        build = lambda cfg: MODEL_DICT[cfg["name"]](**{k: v for k, v in cfg.items() if k != "name"})
        if phase == Phase.TRAIN or inference == "netG_A":
            self.netG_A = build(netG_A_config)
        if phase == Phase.TRAIN or inference == "netG_B":
            self.netG_B = build(netG_B_config)
        if phase == Phase.TRAIN:
            self.netD_A = build(netD_A_config)
            self.netD_B = build(netD_B_config)
            self.fake_A_pool = ImagePool(pool_size)
            self.fake_B_pool = ImagePool(pool_size)

    def initialize_model_and_optimizer(self, init_mini_batch: dict, init_weights: Callable, config: dict, args, scaler,
                                       phase: Phase = Phase.TRAIN):
        if phase != Phase.TEST:
            tr = config[Phase.TRAIN]
            self.loss_name_criterionGAN = tr["loss_criterionGAN"]
            self.loss_name_criterionCycle = tr["loss_criterionCycle"]
            self.loss_name_criterionIdt = tr["loss_criterionIdt"]
            self.criterionGAN = get_loss_function_by_name(self.loss_name_criterionGAN, config)
            self.criterionCycle = get_loss_function_by_name(self.loss_name_criterionCycle, config)
            self.criterionIdt = get_loss_function_by_name(self.loss_name_criterionIdt, config)
            # the step is written for the losses of the reference's experiment (models/gan_loss.py); another criterion is an error, not
            # a silent change of what is optimised
            if phase == Phase.TRAIN and not (isinstance(self.criterionGAN, LSGANLoss) and isinstance(self.criterionCycle, nn.L1Loss)
                                             and isinstance(self.criterionIdt, nn.L1Loss)):
                raise NotImplementedError("CycleGAN trains with loss_criterionGAN: LSGANLoss, loss_criterionCycle: L1Loss, loss_criterionIdt: L1Loss; got "
                                          f"{self.loss_name_criterionGAN}, {self.loss_name_criterionCycle}, {self.loss_name_criterionIdt}")
        super().initialize_model_and_optimizer(init_mini_batch, init_weights, config, args, scaler, phase)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return self.netG_A(input) if self.netG_A is not None else self.netG_B(input)

    def inference(self, mini_batch: Dict[str, Any], post_transformations: Dict[str, Callable], device: torch.device = "cpu",
                  phase: Phase = Phase.TEST) -> Tuple[Output, Dict[str, torch.Tensor]]:
        assert phase == Phase.VALIDATION or phase == Phase.TEST, "This inference function only supports val and test. Use perform_step for training"
        input: torch.Tensor = mini_batch["image"].to(device=device, non_blocking=True)
        pred = self.forward(input)
        losses = dict()
        outputs: Output = {"prediction": [post_transformations["prediction"](i) for i in decollate_batch(pred[0:1, 0:1])]}
        if self.netG_B is not None and phase == Phase.VALIDATION:
            labels: torch.Tensor = mini_batch["label"].to(device=device, non_blocking=True)
            outputs["label"] = [post_transformations["label"](i) for i in decollate_batch(labels[0:1, 0:1])]
            losses[self.loss_name_criterionCycle] = self.criterionCycle(pred.float(), labels.float())
        return outputs, losses

    def _d_loss(self, netD: nn.Module, real: torch.Tensor, pooled_fake: torch.Tensor, batched: bool):
        """(LSGAN(D(real), 1) + LSGAN(D(fake), 0)) / 2 and its backward pass; batched: from one pass over (real | fake)."""
        n = real.shape[0]
        with self.autocast():
            if batched:
                d = netD(torch.cat((real, pooled_fake.detach()), dim=0))
                d_real, d_fake = d[:n], d[n:]
            else:
                d_real, d_fake = netD(real), netD(pooled_fake.detach())
            loss, _ = gan_loss.lsgan([(d_real, True, 0.5), (d_fake, False, 0.5)])
        with self.backward_scope():
            loss.backward()
        return loss

    def perform_training_step(self, mini_batch: Dict[str, Any], scaler, post_transformations: Dict[str, Callable],
                              device: torch.device = "cpu") -> Tuple[Output, Dict[str, float]]:
        real_A: torch.Tensor = mini_batch["real_A"].to(device, non_blocking=True)
        real_B: torch.Tensor = mini_batch["real_B"].to(device, non_blocking=True)
        bg = mini_batch["background"].to(device, non_blocking=True) if "background" in mini_batch else torch.rand_like(real_A)
        u = torch.zeros_like(real_A).uniform_(0, 1)
        nA, nB = real_A.shape[0], real_B.shape[0]
        idt = self.lambda_idt > 0
        batched = real_A.is_cuda if USE_BATCHED_PASSES is None else bool(USE_BATCHED_PASSES)
        # ---- generators: three launch sequences (batched) or the reference's six passes
        with self.autocast():
            mixed_A = gan_loss.mix_max(real_A, bg, u)
            if not batched:
                fake_B = self.netG_A(mixed_A)
                rec_A = self.netG_B(fake_B)
                fake_A = self.netG_B(real_B)
                idt_A = self.netG_A(real_B) if idt else None
                idt_B = self.netG_B(real_A) if idt else None
            elif idt:
                ga = self.netG_A(torch.cat((mixed_A, real_B), dim=0))
                fake_B, idt_A = ga[:nA], ga[nA:]
                gb = self.netG_B(torch.cat((fake_B, real_B, real_A), dim=0))
                rec_A, fake_A, idt_B = gb[:nA], gb[nA:nA + nB], gb[nA + nB:]
            else:
                fake_B, idt_A, idt_B = self.netG_A(mixed_A), None, None
                gb = self.netG_B(torch.cat((fake_B, real_B), dim=0))
                rec_A, fake_A = gb[:nA], gb[nA:]
            rec_B = self.netG_A(gan_loss.mix_max(fake_A, bg, u))
            # ---- generator update against the frozen, not yet updated discriminators
            self.netD_A.requires_grad_(False)
            self.netD_B.requires_grad_(False)
            self.zero_grads("optimizer_G")
            loss_gan, gan_terms = gan_loss.lsgan([(self.netD_A(fake_B), True, 1.0), (self.netD_B(fake_A), True, 1.0)])
            terms = [(rec_A, real_A, self.lambda_A), (rec_B, real_B, self.lambda_B)]
            if idt:
                terms += [(idt_A, real_B, self.lambda_B * self.lambda_idt), (idt_B, real_A, self.lambda_A * self.lambda_idt)]
            loss_l1, l1_terms = gan_loss.l1_pairs(terms)
            loss_G = loss_gan + loss_l1
        with self.backward_scope():
            loss_G.backward()
        self.exchange_gradients("optimizer_G")
        self.optimizer_G.step()
        # ---- discriminator update: pool_B before pool_A, two backward passes, one step
        self.netD_A.requires_grad_(True)
        self.netD_B.requires_grad_(True)
        self.zero_grads("optimizer_D")
        loss_D_A = self._d_loss(self.netD_A, real_B, self.fake_B_pool.query(fake_B), batched)
        loss_D_B = self._d_loss(self.netD_B, real_A, self.fake_A_pool.query(fake_A), batched)
        self.exchange_gradients("optimizer_D")
        self.optimizer_D.step()

        pt = post_transformations or {}
        pp = pt.get("prediction") or (lambda t: t)
        pl = pt.get("label") or (lambda t: t)
        outputs: Output = {
            "prediction": [pp(i) for i in decollate_batch(rec_A[0:1, 0:1].detach())],
            "label": [pl(i) for i in decollate_batch(real_A[0:1, 0:1])],
            "fake_B": fake_B[0:1, 0:1].detach(),
            "idt_A": idt_A[0:1, 0:1].detach() if idt else None,
            "real_B_seg": fake_A[0:1, 0:1].detach(),
        }
        zero = torch.zeros((), device=real_A.device)
        losses = LossValues({"G": loss_G.detach(), "G_A": gan_terms[0], "G_B": gan_terms[1], "D_A": loss_D_A.detach(), "D_B": loss_D_B.detach(),
                             "cycle_A": l1_terms[0], "cycle_B": l1_terms[1], "idt_A": l1_terms[2] if idt else zero, "idt_B": l1_terms[3] if idt else zero})
        return outputs, losses

    def plot_sample(self, visualizer, mini_batch: Dict[str, Any], outputs: Output, *, suffix: str = ""):
        if "fake_B" in outputs:
            return visualizer.plot_gan_seg_sample(mini_batch["real_A"][0], outputs["fake_B"][0], outputs["prediction"][0], mini_batch["real_B"][0],
                                                  None if outputs["idt_A"] is None else outputs["idt_A"][0], outputs["real_B_seg"][0],
                                                  path_A=mini_batch["real_A_path"][0], path_B=mini_batch["real_B_path"][0], suffix=suffix)
        return visualizer.plot_sample(mini_batch["image"][0], outputs["prediction"][0], outputs["label"][0],
                                      path=mini_batch["image_path"][0], suffix=suffix)
