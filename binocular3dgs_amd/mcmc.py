"""Fixed-budget training: the strategy of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., NeurIPS 2024)
in place of clone / split / prune (densify.py).

    relocate      dead Gaussians (opacity <= min_opacity) move onto live ones sampled in proportion to opacity; opacity and
                  scale of source and copies are corrected so that the render does not change.  No host read.
    grow          the set grows by 5 % per call up to a cap the caller names: P is constant once the cap is reached.
    inject_noise  after every optimiser step, covariance-shaped noise on the positions of low-opacity Gaussians: ONE launch.
    McmcSchedule  schedule.IterationSchedule with the strategy swapped; `python -m binocular3dgs_amd.train --densify mcmc
                  --cap_max N` drives it.

All randomness is Philox4x32-10 keyed by (seed, iteration) (include/b3gs_raster.h states which counter serves which output,
tests/mcmc_ref.py restates it): a run is a function of its seed, and an iteration can be repeated later with the same draws.
The noise takes stream 0 with offset = iteration, relocate stream 1 with offset = iteration, grow stream 1 with offset =
iteration | 2^31.

One departure from the paper's code: the Adam moments of EVERY row written -- the sampled sources and their copies -- are set
to zero (the paper's code zeroes the sources only and leaves the stale moments of the dead rows in place).
step.ShardedAdam is not supported: its moments are sharded over the ranks.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _lib
from .densify import _ATTRS, _adam_state, _rebind_optimizer
from .schedule import IterationSchedule

N_MAX = 51
GROW_OFFSET = 1 << 31
_M64 = (1 << 64) - 1


def _C():
    from . import _C as mod
    return mod


def random_words(n: int, seed: int, stream_id: int, offset: int, device="cuda") -> torch.Tensor:
    """n raw Philox words as int32 (the bits of uint32) on the device"""
    return _C().mcmc_random(int(n), int(seed) & _M64, int(stream_id), int(offset), 0, torch.device(device))


def random_normals(n: int, seed: int, stream_id: int, offset: int, device="cuda") -> torch.Tensor:
    """n standard normals (float32) on the device"""
    return _C().mcmc_random(int(n), int(seed) & _M64, int(stream_id), int(offset), 1, torch.device(device))


def _on_device(model, what):
    if not model._xyz.is_cuda:
        raise _lib.B3gsError(f"{what} needs the model on the HIP device (no CPU fallback)")


def inject_noise(model, lr_xyz, *, iteration: int, seed: int, noise_lr: float = 5e5, normals: Optional[torch.Tensor] = None) -> None:
    """xyz += Sigma n g (noise_lr lr_xyz), g = 1 / (1 + exp(100 (opacity - 0.005))), in place, one launch.
    lr_xyz: a float, or ONE float32 on the device.  normals: None (drawn in registers for (seed, iteration)) or [P,3]."""
    _on_device(model, "inject_noise")
    lr_dev = lr_xyz if torch.is_tensor(lr_xyz) else None
    with torch.no_grad():
        _C().mcmc_noise(model._xyz.detach(), model._scaling.detach(), model._rotation.detach(), model._opacity.detach(), normals,
                        int(seed) & _M64, int(iteration), float(noise_lr), 0.0 if lr_dev is not None else float(lr_xyz), lr_dev)


def _moments(optimizer, params):
    if optimizer is not None and hasattr(optimizer, "gather_full_state"):
        raise _lib.B3gsError("mcmc: step.ShardedAdam is not supported -- its moments are sharded over the ranks, relocation "
                             "zeroes rows of all of them; use optim.Adam or step.FusedAdam")
    m, v = _adam_state(optimizer, params)
    return (m, v) if m is not None else ([], [])


def relocate(model, optimizer, *, iteration: int, seed: int, min_opacity: float = 0.005, debug: bool = False,
             draws: Optional[torch.Tensor] = None):
    """In place; no host read.  debug=True -> (src, count, rank, weight_scan, head) as tensors (src -1: not relocated;
    head = total weight, dead rows, status).  draws (debug): int64 [P], the bits of the 64-bit draws by dead rank."""
    _on_device(model, "relocate")
    params = [getattr(model, a) for a in _ATTRS]
    m, v = _moments(optimizer, params)
    with torch.no_grad():
        out = _C().mcmc_relocate([p.detach() for p in params], list(m), list(v), params[0].shape[0], float(min_opacity), N_MAX,
                                 int(seed) & _M64, int(iteration), draws, bool(debug))
    return out if debug else None


def grow(model, optimizer, cap_max: int, *, iteration: int, seed: int, rate: float = 0.05, min_opacity: float = 0.005) -> int:
    """new_P = min(cap_max, int((1 + rate) P)): new tensors, the old rows copied, the appended rows filled by the relocation
    kernels (sampled over all old rows); the optimiser is re-bound as densify does.  -> the new P (no host read: P is known)."""
    _on_device(model, "grow")
    params = [getattr(model, a) for a in _ATTRS]
    P = params[0].shape[0]
    new_P = min(int(cap_max), int((1.0 + rate) * P))
    if new_P <= P:
        return P
    m_in, v_in = _moments(optimizer, params)
    dev = params[0].device
    widths = [p.numel() // P for p in params]
    with torch.no_grad():
        new = []
        for p in params:
            t = torch.zeros((new_P,) + tuple(p.shape[1:]), dtype=torch.float32, device=dev)
            t[:P] = p.detach()
            new.append(t)
        flat_m = flat_v = None
        nm, nv = [], []
        if m_in:
            tot = sum(new_P * w for w in widths)
            flat_m, flat_v = torch.zeros(tot, dtype=torch.float32, device=dev), torch.zeros(tot, dtype=torch.float32, device=dev)
            off = 0
            for t, w in enumerate(widths):
                nm.append(flat_m[off:off + new_P * w])
                nv.append(flat_v[off:off + new_P * w])
                nm[-1][:P * w] = m_in[t].reshape(-1)
                nv[-1][:P * w] = v_in[t].reshape(-1)
                off += new_P * w
        _C().mcmc_relocate(new, nm, nv, P, float(min_opacity), N_MAX, int(seed) & _M64, (int(iteration) | GROW_OFFSET) & 0xFFFFFFFF,
                           None, False)
    new_params = [nn.Parameter(t, requires_grad=True) for t in new]
    for a, p in zip(_ATTRS, new_params):
        setattr(model, a, p)
    model.xyz_gradient_accum = torch.zeros((new_P, 1), device=dev)
    model.denom = torch.zeros((new_P, 1), device=dev)
    model.max_radii2D = torch.zeros((new_P,), device=dev)
    if optimizer is not None:
        _rebind_optimizer(optimizer, params, new_params, flat_m, flat_v, widths, new_P)
    return new_P


class McmcSchedule(IterationSchedule):
    """The iteration of schedule.IterationSchedule with the strategy swapped: the loss gains opacity_reg mean(opacity) +
    scale_reg mean(scaling); no densification statistics; relocate then grow every densification_interval after
    densify_from_iter and before densify_until_iter; inject_noise after optimizer.step() with that iteration's position
    learning rate.  The opacity decay stays under the caller's switch (opacity_decay_factor=None: off) and does not
    extend the window."""
    keeps_stats = False
    decay_extends_densification = False

    def __init__(self, model, scene, pipe, background, *, cap_max: int, seed: int = 0, noise_lr: float = 5e5, opacity_reg: float = 0.01,
                 scale_reg: float = 0.01, log_relocations: bool = False, **kw):
        super().__init__(model, scene, pipe, background, **kw)
        if cap_max is None or int(cap_max) < 1:
            raise ValueError("McmcSchedule: cap_max, the final number of Gaussians, is at least 1")
        self.cap_max, self.seed, self.noise_lr = int(cap_max), int(seed), float(noise_lr)
        self.opacity_reg, self.scale_reg = float(opacity_reg), float(scale_reg)
        # log_relocations: keep (src, count, rank, weight_scan, head) of every relocate() as device tensors, by iteration
        self.log_relocations, self.relocation_log = bool(log_relocations), {}

    def _add_loss_terms(self, total):
        m = self.model
        return total + (self.opacity_reg * m.get_opacity.mean() + self.scale_reg * m.get_scaling.mean())

    def _densify(self, it):
        m = self.model
        P = m.get_xyz.shape[0]
        out = relocate(m, m.optimizer, iteration=it, seed=self.seed, min_opacity=self.min_opacity, debug=self.log_relocations)
        if self.log_relocations:
            self.relocation_log[it] = out
        self.densified = grow(m, m.optimizer, self.cap_max, iteration=it, seed=self.seed, min_opacity=self.min_opacity) != P

    def _after_step(self, it, lr_xyz):
        inject_noise(self.model, lr_xyz, iteration=it, seed=self.seed, noise_lr=self.noise_lr)
