"""Development aid: the N-channel output head (csrc/head.hip) + the fused Dice + BCE loss at the 3-D reconstruction set-up's shape
(B = 4, 1216^2, 32 -> 44), against the path they replace, timed in the same run: hipBLASLt GEMM + bias + permute().contiguous() and
the torch loss expression. OCTA_STRICT=0 for the latter (it is the vendor fallback). Then the whole training step of
configs/config_3d_recon_supervised.yml's network (DynUNet to --cout channels, Adam, the config's post-processing of the scored sample) on
device-resident random batches, with the new head + fused loss and with the old chain. `--size 304` for a quick look."""
import argparse
import os
import sys
os.environ["OCTA_STRICT"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from octa_autosegmentation_amd.models import losses, mfma_conv, networks


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--size", type=int, default=1216)
ap.add_argument("--cin", type=int, default=32)
ap.add_argument("--cout", type=int, default=44)
args = ap.parse_args()
B, S, CIN, COUT = args.batch, args.size, args.cin, args.cout
npix = B * S * S
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.randn(B, S, S, CIN, device="cuda", generator=g).bfloat16().requires_grad_(True)
w = (torch.randn(COUT, CIN, 1, 1, device="cuda", generator=g) * 0.2).requires_grad_(True)
bias = torch.randn(COUT, device="cuda", generator=g).requires_grad_(True)
tgt = (torch.rand(B, COUT, S, S, device="cuda", generator=g) > 0.7).float()
loss_fn = losses.DiceBCELoss(True)


def new_head():
    return mfma_conv.conv1x1_bias_nhwc(x, w, bias)


def old_head():
    with networks.vendor_reference():          # the GEMM path without the fallback warning
        return mfma_conv.conv1x1_bias_nhwc(x, w, bias).permute(0, 3, 1, 2).contiguous()


def new_loss(y):
    return loss_fn(y, tgt)


def old_loss(y):
    return (loss_fn.dice(y, tgt) + loss_fn.bce(y, tgt)) / 2


def step(head, loss):
    for t in (x, w, bias):
        t.grad = None
    loss(head().float()).backward()             # .float(): as models/lambda_model.py hands the logits to the loss


y_new, y_old = new_head(), old_head()
dy = torch.randn_like(y_new)
fwd_bytes, bwd_bytes = npix * (2 * CIN + 2 * COUT), npix * (2 * CIN + 2 * COUT + 2 * CIN)
print(f"shape: B = {B}, {S} x {S}, {CIN} -> {COUT}; {2 * CIN + 2 * COUT} B/pixel forward, {4 * CIN + 2 * COUT} B/pixel backward")
for name, head, y in (("head.hip", new_head, y_new), ("GEMM + bias + permute().contiguous()", old_head, y_old)):
    t_f = timed(head)
    t_b = timed(lambda: torch.autograd.grad(y, (x, w, bias), dy, retain_graph=True))
    print(f"{name}: forward {t_f:.3f} ms ({fwd_bytes / t_f / 1e9:.2f} TB/s of the byte count), backward {t_b:.3f} ms ({bwd_bytes / t_b / 1e9:.2f} TB/s)")
del y_new, y_old, dy
t_new = timed(lambda: step(new_head, new_loss), reps=5)
t_old = timed(lambda: step(old_head, old_loss), reps=5)
print(f"head + loss, forward + backward: head.hip + fused loss {t_new:.3f} ms | GEMM chain + torch loss {t_old:.3f} ms")

# ---- the training step of the cut-down config (no loader: random device-resident batches) ------------------------------------------------
del x, w, bias
torch.cuda.empty_cache()
import yaml
from octa_autosegmentation_amd.data.image_dataset import get_post_transformation
from octa_autosegmentation_amd.models.segmentation_trainer import SegmentationTrainer
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "config_3d_recon_supervised.yml")) as f:
    cfg = yaml.safe_load(f)
cfg["General"]["model"]["out_channels"] = COUT
cfg["General"]["seed"] = 1
post = get_post_transformation(cfg, "Train")
trainer = SegmentationTrainer(cfg, "cuda:0")
batch = {"image": (torch.rand(B, 1, S, S, device="cuda", generator=g) > 0.8).to(torch.bfloat16), "label": tgt.to(torch.bfloat16)}


def train_step():
    trainer.perform_training_step(batch, None, post)


t_new = timed(train_step, reps=5)
losses.USE_FUSED_LOSS = False
with networks.vendor_reference():
    t_old = timed(train_step, reps=5)
losses.USE_FUSED_LOSS = True
print(f"training step, B = {B}, {S} x {S}, {COUT} channels: {t_new:.2f} ms | with the GEMM head and the torch loss {t_old:.2f} ms")
