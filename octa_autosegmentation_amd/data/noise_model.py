"""The reference's handcrafted noise model (models/noise_model.py NoiseModel / ControlPointBetaNoise with adversarial=False, used by
data/data_transforms.py NoiseModeld): the random draws in the reference's order from torch's GLOBAL CPU generator, and the arithmetic restated
on torch for host tensors. The device form of the arithmetic and of the per-pixel draws is csrc/noise_model.hip (data/gpu_augment.py
noise_model); it takes the control grids drawn here.

Per call, for a mini-batch of n images, the reference draws
  * the vessel noise's control points: alpha then beta, each 10^(2 x - 1) with x = Beta(2, 2).sample((n, 1, gh, gw));
  * the speckle noise's control points, the same way;
  * the gamma control points, uniform_(0, 1) on an (n, 1, gh, gw) tensor of the image's dtype.
The FIRST call of an instance draws all of that twice and uses the second set: the reference initialises its parameters with a full draw
when it creates its optimiser, then redraws them like in every later call.

Then per pixel: A, B = max(bicubic(control points), 1e-3); Delta ~ Beta(A_v, B_v); N ~ Beta(A_s, B_s);
Gamma = bicubic(clamp(g, 0, 1) 2 lambda_gamma + (1 - lambda_gamma));
out = pow(max(I, I_d lambda_delta Delta) (lambda_speckle N + 1 - lambda_speckle) + 1e-6, Gamma), between two bilinear resamples by
1 / downsample_factor and back that are identities at downsample_factor 1.
"""
import torch
import torch.nn.functional as F


class NoiseModelDraws:
    """The state the reference's NoiseModel keeps between calls, as far as the non-adversarial path has any: whether the first call's
    extra set of control points has been drawn, and the shape / dtype its parameters were created with."""

    def __init__(self, grid_size=(9, 9)):
        self.grid_size = tuple(int(v) for v in grid_size)
        self.shape = None            # (n, 1, gh, gw) of the first call: the reference's parameters keep it
        self.gamma_dtype = None

    def _one_set(self):
        sampler = torch.distributions.beta.Beta(2, 2)
        grids = [10 ** (sampler.sample(self.shape) * 2 - 1) for _ in range(4)]      # alpha_v, beta_v, alpha_s, beta_s
        grids.append(torch.zeros(self.shape, dtype=self.gamma_dtype).uniform_(0, 1))
        return grids

    def control_points(self, n_batch, dtype=torch.float32):
        """[alpha_v, beta_v, alpha_s, beta_s, gamma], each (n, 1, gh, gw), drawn from torch's global generator."""
        if self.shape is None:
            self.shape, self.gamma_dtype = (int(n_batch), 1) + self.grid_size, dtype
            self._one_set()          # the initialisation draw, overwritten before it is used
        return self._one_set()


def noise_model_host(I, I_d, grids, lambda_delta=1, lambda_speckle=0.7, lambda_gamma=0.3, downsample_factor=1):  # noqa: E741
    """The reference's arithmetic on host tensors I, I_d [n, 1, H, W] with the control points `grids` of NoiseModelDraws.control_points;
    the two per-pixel Beta fields come from torch's global generator (Delta first, then N)."""
    size = list(I.shape[2:])
    n = I.shape[0]
    x = F.interpolate(I, scale_factor=1 / downsample_factor, mode="bilinear")
    h, w = x.shape[-2:]

    def beta_field(alpha, beta):
        A = torch.clamp(F.interpolate(alpha, (h, w), mode="bicubic"), min=1e-3)
        B = torch.clamp(F.interpolate(beta, (h, w), mode="bicubic"), min=1e-3)
        return torch.distributions.beta.Beta(A, B).rsample()[:n]

    Delta = beta_field(grids[0], grids[1])
    N = beta_field(grids[2], grids[3])
    Gamma = F.interpolate((torch.clamp(grids[4], 0, 1) * (2 * lambda_gamma) + (1 - lambda_gamma))[:n], (h, w), mode="bicubic")
    x = torch.maximum(x, I_d * lambda_delta * Delta)
    x = x * (lambda_speckle * N + (1 - lambda_speckle))
    x = torch.pow(x + 1e-6, Gamma)
    return F.interpolate(x, size=size, mode="bilinear")


def nearest_roundtrip_tables(spatial, factor):
    """Per spatial axis the source index of every output element of
    interpolate(interpolate(x, scale_factor=factor), size=spatial) (both `nearest`): the two resamples of RandomDecreaseResolutiond as ONE
    gather. The tables are made by torch's own CPU nearest kernel on an index ramp, so they are its index arithmetic by construction."""
    tables = []
    for n in spatial:
        ramp = torch.arange(int(n), dtype=torch.float32).view(1, 1, -1)
        tables.append(F.interpolate(F.interpolate(ramp, scale_factor=factor), size=int(n)).view(-1).to(torch.int64))
    return tables
