"""Training / validation metrics of the entry points (reference utils/metrics.py:165-196 MetricsManager): DSC and IoU in
the training phase; the validation phase adds clDice, AUC, ACC, Recall and Precision, in the reference's order. Every score is computed
on the device the tensors live on and read back as ONE scalar per metric and sample; the reference moves whole 1216x1216
maps to numpy for each of them. clDice's skeletons are a kernel of their own (csrc/skeleton.hip through utils/skeleton.py, DESIGN.md
4.2k); the other scores are torch reductions -- logging quantities, not a kernel target."""
import math

import torch

from .aside import join_aside
from .enums import Phase


class Metric:
    """Scores are kept as 0-dim tensors ON THE DEVICE of the maps (NaN = "skip this sample", e.g. empty ground truth) and meet in
    one stacked nanmean when the epoch ends: a training step queues no host read of its own (the reference reads every score of
    every sample back as a python float)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.scores = []

    def add(self, value):
        self.scores.append(value if torch.is_tensor(value) else torch.tensor(float(value)))

    def aggregate(self) -> torch.Tensor:
        if not self.scores:
            return torch.tensor(float("nan"))
        dev = next((s.device for s in self.scores if s.is_cuda), torch.device("cpu"))
        join_aside(dev)                  # scores of training steps are computed on the side stream (utils/aside.py)
        v = torch.stack([s.detach().to(dev, torch.float64).reshape(()) for s in self.scores])
        ok = ~torch.isnan(v)
        n = ok.sum()
        mean = torch.where(ok, v, torch.zeros_like(v)).sum() / n.clamp(min=1)
        return torch.where(n > 0, mean, torch.full_like(mean, float("nan"))).float().cpu()


def _flat_bool(t):
    return t.detach().reshape(-1) != 0


def _nan_unless(cond, value):
    return torch.where(cond, value, torch.full_like(value, float("nan")))


class MacroDiceMetric(Metric):
    """Per layer 2 |gt & pred| / (|gt| + |pred|) for class 1, NaN (skipped) for an empty ground truth (metrics.py:95-123)."""

    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            for layer in range(len(p_i)):
                gt, pr = y_i[layer].detach().float(), p_i[layer].detach().float()
                gsum = gt.sum()
                inter = ((gt == 1) & (pr == 1)).sum()
                self.add(_nan_unless(gsum != 0, 2.0 * inter / (gsum + pr.sum())))

    def aggregate(self):
        return super().aggregate() if self.scores else torch.tensor(0)


class MeanIoU(Metric):
    """MONAI MeanIoU(include_background=True, reduction='mean') on binarised maps: per channel |p & y| / |p | y|; channels with
    an empty ground truth are NaN and ignored (MONAI's ignore_empty default)."""

    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            for c in range(len(p_i)):
                p, g = _flat_bool(p_i[c]), _flat_bool(y_i[c])
                self.add(_nan_unless(g.any(), (p & g).sum().double() / (p | g).sum().clamp(min=1).double()))


class _Confusion(Metric):
    def counts(self, p_i, y_i):
        """(tp, tn, fp, fn) as float64 0-dim tensors on the maps' device."""
        p, g = _flat_bool(p_i), _flat_bool(y_i)
        tp, pp, gp = (p & g).sum().double(), p.sum().double(), g.sum().double()
        n = float(p.numel())
        return tp, n - pp - gp + tp, pp - tp, gp - tp


class AccuracyMetric(_Confusion):
    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            tp, tn, fp, fn = self.counts(p_i, y_i)
            self.add((tp + tn) / (tp + tn + fp + fn))


class Recall(_Confusion):
    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            tp, tn, fp, fn = self.counts(p_i, y_i)
            self.add(_nan_unless(tp + fn > 0, tp / (tp + fn).clamp(min=1)))


class Precision(_Confusion):
    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            tp, tn, fp, fn = self.counts(p_i, y_i)
            self.add(_nan_unless(tp + fp > 0, tp / (tp + fp).clamp(min=1)))


class AUCMetric(Metric):
    """ROC AUC of the flattened map (monai.metrics.compute_roc_auc): rank statistic with average ranks for ties."""

    def __call__(self, y_pred, y):
        for p_i, y_i in zip(y_pred, y):
            s, g = p_i.detach().reshape(-1).double(), _flat_bool(y_i)
            n_pos = g.sum().double()
            n_neg = float(g.numel()) - n_pos
            vals, inv, cnt = torch.unique(s, sorted=True, return_inverse=True, return_counts=True)
            hi = torch.cumsum(cnt, 0).double()
            avg_rank = hi - (cnt.double() - 1) / 2          # average 1-based rank of each distinct score
            r_pos = (avg_rank[inv] * g.double()).sum()
            auc = (r_pos - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg).clamp(min=1)
            self.add(_nan_unless((n_pos > 0) & (n_neg > 0), auc))


class ClDiceMetric(Metric):
    """clDice per sample and layer as the reference's utils/cldice.py:19-35: with s = skeleton (utils/skeleton.py, Zhang-Suen),
    tprec = sum(v_p * s_l) / sum(s_l), tsens = sum(v_l * s_p) / sum(s_p) -- `v` enters by VALUE, not as a mask --
    clDice = 2 tprec tsens / (tprec + tsens), 0 / 0 = NaN as numpy gives it (skipped by `aggregate`, the reference's nanmean). The sums
    are float64 (the reference sums in the maps' dtype, which is the same number for 0 / 1 maps of up to 2^24 pixels).
    CUDA maps: both skeletons of a sample come from ONE batched call of the kernel (csrc/skeleton.hip), the four sums are device
    reductions and the score stays a 0-dim device tensor; the only host reads are the kernel's chunked convergence flags. CPU maps take
    `skeletonize_host`. No CUDA tensor ever takes the host path, so there is nothing to route through the loud-fallback door.
    3-D layers (the reference's `method="lee"` branch; no config here produces them) raise NotImplementedError.
    Parity with scikit-image itself is UNPINNED (it is neither installed here nor shipped with the reference): the rule is pinned by
    the published algorithm, the literal oracle of tests/test_skeleton.py and the known answers there."""

    def __call__(self, y_pred, y):
        from .skeleton import skeletonize
        for p_i, y_i in zip(y_pred, y):
            for layer in range(len(p_i)):
                v_p, v_l = p_i[layer].detach(), y_i[layer].detach()
                if v_p.dim() != 2:
                    raise NotImplementedError(f"clDice of a {v_p.dim()}-D layer (shape {tuple(v_p.shape)}): only the 2-D skeleton is implemented, "
                                              "the reference's 3-D skeletonize(method='lee') is not")
                dt = torch.promote_types(v_p.dtype, v_l.dtype)          # non-zero stays non-zero; the skeleton takes any dtype
                s_p, s_l = skeletonize(torch.stack([v_p.to(dt), v_l.to(dt)])).double()
                tprec = (v_p.double() * s_l).sum() / s_l.sum()
                tsens = (v_l.double() * s_p).sum() / s_p.sum()
                self.add(2 * tprec * tsens / (tprec + tsens))


class MetricsManager:
    def __init__(self, phase: Phase = Phase.TRAIN):
        self.metrics = {"DSC": MacroDiceMetric(), "IoU": MeanIoU()}
        if phase != Phase.TRAIN:
            self.metrics.update({"ClDice": ClDiceMetric(), "AUC": AUCMetric(), "ACC": AccuracyMetric(), "Recall": Recall(), "Precision": Precision()})
        self.comp = "DSC"

    def __call__(self, y_pred, y):
        for v in self.metrics.values():
            v(y_pred=y_pred, y=y)

    def aggregate_and_reset(self, prefix: str = ""):
        d = dict()
        for k, v in self.metrics.items():
            d[f"{prefix}_{k}"] = v.aggregate().item()
            v.reset()
        return d

    def get_comp_metric(self, prefix: str):
        return f"{prefix}_{self.comp}"
