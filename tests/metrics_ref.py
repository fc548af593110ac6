"""The PyTorch statement of b3gs_image_metrics_batch (csrc/metrics.hip), on the CPU: the formula of
tests/test_gpu_evaluate.py::test_metrics_are_deterministic_and_cover_every_pixel as a helper, for every mode, channel count
and mask shape.

The prepared pair is float32 and must be reproduced bit for bit: clamp, the 8-bit round trip and the mask composite are
separate float32 operations here as they are in the kernel (-ffp-contract=off).  It runs on the CPU because the round trip
divides by 255 (torch's device kernel multiplies by the reciprocal instead).  The sums are float64 sums of the float32
differences, so only the order of the additions differs from the kernel's."""
import torch

CLAMP, QUANTIZE = 1, 2


def prepare(x, mode):
    """float32 CPU tensor -> what the kernel compares: clamp to [0, 1] (a NaN stays), then uint8(clamp(x * 255 + 0.5, 0, 255)) / 255."""
    if mode & CLAMP:
        x = x.clamp(0, 1)
    if mode & QUANTIZE:
        x = torch.clamp(x * 255 + 0.5, 0, 255).to(torch.uint8).to(torch.float32) / 255
    return x


def reference(imgs, gts, masks, mode):
    """-> (sums float64 [n, 2C + 2], prepared image, prepared gt: float32 [n, C, H, W]), all on the CPU.
    Row: sum |d| per channel, sum d^2 per channel, sum d^2 where mask == 1, the count of those entries; no mask = all ones.
    masks: None, or one [1, H, W] / [C, H, W] tensor per view."""
    r = prepare(torch.stack([t.detach().float().cpu() for t in imgs]), mode)
    q = prepare(torch.stack([t.detach().float().cpu() for t in gts]), mode)
    if masks is None:
        one = torch.ones_like(r, dtype=torch.bool)
    else:
        m = torch.stack([t.detach().float().cpu() for t in masks])
        r, q = r * m + (1 - m), q * m + (1 - m)
        one = (m == 1).expand_as(r)
    d = (r - q).double()
    zero = torch.zeros((), dtype=torch.float64)
    sums = torch.cat([d.abs().sum((2, 3)), (d * d).sum((2, 3)), torch.where(one, d * d, zero).sum((1, 2, 3))[:, None],
                      one.sum((1, 2, 3))[:, None].double()], 1)
    return sums, r, q
