"""Child process of tests/test_norm_gpu.py::test_image_group_path_in_a_fresh_process: started with OCTA_NORM_CACHE_MB=1 (read once per
process by csrc/norm.hip), it runs the channels-last norm at B = 3, 64 x 64, C = 64 -- forward in image groups of 2 + 1, backward image by
image with cleared dgamma / dbeta and atomics -- and compares with tests/_norm_ref.py. Exit status 0 only if every bound holds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import torch
    import _norm_ref as nr
    from octa_autosegmentation_amd import _native
    from octa_autosegmentation_amd.models import mfma_conv as mc
    assert os.environ.get("OCTA_NORM_CACHE_MB") == "1"
    gen = torch.Generator().manual_seed(3164)
    B, H, W, C = 3, 64, 64, 64
    x = (torch.randn(B, H, W, C, generator=gen) * 2.0 + 0.7).to(torch.bfloat16).cuda()
    dy = torch.randn(B, H, W, C, generator=gen).to(torch.bfloat16).cuda()
    w, b = (torch.rand(C, generator=gen) + 0.5).cuda(), (0.5 * torch.randn(C, generator=gen)).cuda()
    xm, wm, bm = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = mc.instance_norm_leaky_relu_nhwc(xm, wm, bm, 0.01, nr.EPS)
    y.backward(dy)
    mean, rstd = torch.empty(B * C, dtype=torch.float32, device="cuda"), torch.empty(B * C, dtype=torch.float32, device="cuda")
    y2 = torch.empty_like(x)
    _native.launch("octa_instnorm_lrelu_nhwc_fwd", x.device, x, y2, w, b, mean, rstd, B, C, H * W, 0.01, nr.EPS, None, 0, None, 0)
    r = nr.reference(nr.bnc(x, "nhwc"), w, b, 0.01, nr.EPS, dy=nr.bnc(dy, "nhwc"))
    rat = nr.ratios(r, nr.bounds(r), dict(y=nr.bnc(y.detach(), "nhwc"), dx=nr.bnc(xm.grad, "nhwc"), dgamma=wm.grad, dbeta=bm.grad, mean=mean, rstd=rstd))
    print("RATIO image groups", {k: float(f"{v:.4g}") for k, v in rat.items()})
    nr.assert_within(rat, "image groups")
    nr.assert_within(nr.ratios(r, nr.bounds(r), dict(y=nr.bnc(y2, "nhwc"))), "image groups (entry point)")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
