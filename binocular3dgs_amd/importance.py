"""Which Gaussians carry the renders: per-Gaussian render contribution over a camera set, scores, selection, pruning.

contributions() renders the cameras as evaluate.py does (up to 8 views of one W x H per b3gs_forward_raw_batch launch on the
evaluation-owned FusedRasterizer, no gradients, one-round binning, the full 32-bit depth sort) and, after every launch, walks
the tile lists that forward left on the device a second time (b3gs_blend_contribution_batch, csrc/contrib.hip).  Every blended
(pixel, Gaussian) has the weight w = alpha * T, the share of the pixel the Gaussian paints; per Gaussian it returns

    weight    sum of w over the counted pixels of all cameras   (float64; the device sums rint(w 2^32) as integers)
    hits      number of (camera, pixel) it was blended into     (int64)
    dominant  number of (camera, pixel) where its w is the pixel's largest, ties to the nearer one   (int64)
    wmax      its largest w anywhere                            (float32)

All four are integer sums / maxima on the device: the same bits whatever the batch size or the camera order.

One caveat for pruning by hits.  The entry that saturates a pixel (T (1 - alpha) < 1e-4) stops the pixel WITHOUT being blended,
so it gets no hit there.  When it is pruned, the entry behind it is tested in its place and may blend.  Removing the Gaussians
with zero hits therefore leaves the renders of the same cameras bit-identical only where no pixel saturates (final_T stays
above 1e-4 everywhere); elsewhere the change is bounded by the 1e-4 of transmittance that was left.

python -m binocular3dgs_amd.prune is the command line over these functions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

RULES = ("weight", "significance")


@dataclass
class Contributions:
    weight: torch.Tensor     # [P] float64
    hits: torch.Tensor       # [P] int64
    dominant: torch.Tensor   # [P] int64
    wmax: torch.Tensor       # [P] float32


def contributions(model, cameras: Sequence, bg: torch.Tensor, *, masks=None, batch: int = 8,
                  capacity: Optional[int] = None) -> Contributions:
    """The four statistics of every Gaussian of `model` over `cameras`, device tensors [P].
    masks: None, or per camera None or an [H,W] tensor (nonzero / True = count the pixel; a DTU camera's object mask, say)."""
    from . import _C
    from .evaluate import _walk_batches
    if masks is not None and len(masks) != len(cameras):
        raise ValueError("one mask (or None) per camera")
    dev = model.get_xyz.device
    P = model.get_xyz.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    wq = torch.zeros(P, dtype=torch.int64, device=dev)
    hits32, wmax_bits, dom32 = torch.zeros(P, **i32), torch.zeros(P, **i32), torch.zeros(P, **i32)
    # The device counters are 32-bit words: folded into 64-bit sums and zeroed after every launch, so that no camera set can
    # wrap them (one launch counts at most 8 W H pixels).  The weight words are 64-bit already.
    hits, dominant = torch.zeros(P, dtype=torch.int64, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)
    for idx, _outs, W, H, slots in _walk_batches(model, cameras, bg, batch, capacity):
        views = []
        for i, s in zip(idx, slots):
            m = None if masks is None or masks[i] is None else (masks[i].reshape(H, W) != 0).to(device=dev, dtype=torch.uint8)
            views.append((s.geom, s.binning, s.img, W, H, m))
        _C.blend_contribution(views, wq, hits32, wmax_bits, dom32)
        hits += hits32.to(torch.int64) & 0xFFFFFFFF
        dominant += dom32.to(torch.int64) & 0xFFFFFFFF
        hits32.zero_()
        dom32.zero_()
    # (w < 1: the sign bit of its float32 word is clear, the int32 view holds the unsigned word)
    weight = (wq >> 32).to(torch.float64) + (wq & 0xFFFFFFFF).to(torch.float64) / 4294967296.0
    return Contributions(weight=weight, hits=hits, dominant=dominant, wmax=wmax_bits.view(torch.float32))


def score(contrib: Contributions, model, rule: str = "weight") -> torch.Tensor:
    """One float64 number per Gaussian, larger = keep.
    "weight":        the weight sum itself -- the number of pixels' worth of the camera set the Gaussian painted.
    "significance":  hits * sigmoid(opacity) * v^0.1 with v = prod(exp(scaling)) / its 90th percentile, clipped to 1: the global
                     significance score of LightGaussian (Fan et al., "LightGaussian: Unbounded 3D Gaussian Compression with
                     15x Reduction and 200+ FPS", 2023, eq. 3-4), with the hit count of this camera set as its hit count."""
    if rule == "weight":
        return contrib.weight
    if rule == "significance":
        with torch.no_grad():
            vol = torch.prod(model.get_scaling.double(), dim=1)
            P = vol.shape[0]
            if P == 0:
                return vol
            v90 = torch.sort(vol).values[min(int(0.9 * P), P - 1)]
            v = torch.clamp(vol / v90, 0.0, 1.0) ** 0.1
            return contrib.hits.double() * model.get_opacity.double().reshape(-1) * v
    raise ValueError(f"rule must be one of {RULES}")


def select(score, *, keep: Optional[float] = None, min_score: Optional[float] = None, min_hits: Optional[int] = None,
           never_dominant: bool = False, contrib: Optional[Contributions] = None) -> torch.Tensor:
    """Bool mask [P] of the Gaussians to keep; the criteria are ANDed.
    keep:           a fraction -- the top ceil(keep * P) by (score descending, index ascending): ties are decided by index
    min_score:      score >= min_score
    min_hits:       hits >= min_hits                    (needs `contrib`)
    never_dominant: drop the Gaussians that are the largest weight of no pixel   (needs `contrib`)
    `score` may be a Contributions: its weight is the score and it is `contrib`."""
    if isinstance(score, Contributions):
        contrib, score = score, score.weight
    P = score.shape[0]
    mask = torch.ones(P, dtype=torch.bool, device=score.device)
    if keep is not None:
        if not 0.0 <= keep <= 1.0:
            raise ValueError("keep is a fraction in [0, 1]")
        n = min(P, int(math.ceil(keep * P)))
        order = torch.sort(score, descending=True, stable=True).indices
        top = torch.zeros(P, dtype=torch.bool, device=score.device)
        top[order[:n]] = True
        mask &= top
    if min_score is not None:
        mask &= score >= min_score
    if min_hits is not None or never_dominant:
        if contrib is None:
            raise ValueError("min_hits / never_dominant need the Contributions (contrib=...)")
        if min_hits is not None:
            mask &= contrib.hits >= int(min_hits)
        if never_dominant:
            mask &= contrib.dominant > 0
    return mask


def prune(model, mask: torch.Tensor):
    """A new GaussianModel of the rows where `mask` is True, SH degrees carried over.  No optimizer state is touched or made:
    pruning inside a training loop is not what this is for."""
    from .gaussian_model import GaussianModel
    mask = mask.to(device=model._xyz.device, dtype=torch.bool)
    if mask.shape != (model._xyz.shape[0],):
        raise ValueError("one mask element per Gaussian")
    rows = [p.detach()[mask] for p in (model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation,
                                       model._opacity)]
    return GaussianModel.from_tensors(*rows, sh_degree=model.max_sh_degree, active_sh_degree=model.active_sh_degree,
                                      requires_grad=model._xyz.requires_grad)
