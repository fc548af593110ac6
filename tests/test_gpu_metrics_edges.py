"""GPU: b3gs_image_metrics_batch (csrc/metrics.hip) through evaluate.image_metrics against the PyTorch statement
tests/metrics_ref.py, where the kernel's indexing depends on its arguments: 1, 2 and 4 channels (the `c >= C` break and
the fold's slot mapping), every mask shape and mode, more views than the 32 rows of the kernel-argument table (chunks
with view0 > 0), and pixel counts around one workgroup's stride and above the cap of 256 workgroups per view.

Criteria: the count column is exact; the prepared pair equals the float32 statement bit for bit; the sums keep
rel_l2 < 1e-6 over the whole table and 1e-12 relative per entry of every column -- the kernel adds float64 values of the
same float32 differences, so only the order of the additions differs from torch's float64 sum.
Observed on an MI355X, the maximum over all tests of this file of |sum - reference| / reference per column kind:
    sum |d| 0 (exact), sum d^2 2.5e-16, masked sum d^2 2.89e-16, count 0 (exact): one or two ulps of a float64."""
import numpy as np
import pytest
import torch

import metrics_ref
from helpers import rel_l2
from metrics_ref import CLAMP, QUANTIZE

gpu = pytest.mark.gpu
COLUMN_TOL = 1e-12


def test_reference_on_hand_values():
    img, gt, mask = torch.tensor([[[0.5, 2.0]]]), torch.tensor([[[0.25, -1.0]]]), torch.tensor([[[1.0, 0.5]]])
    s, r, q = metrics_ref.reference([img], [gt], [mask], CLAMP)       # r = (0.5, 1 * 0.5 + 0.5), q = (0.25, 0 * 0.5 + 0.5)
    assert r.tolist() == [[[[0.5, 1.0]]]] and q.tolist() == [[[[0.25, 0.5]]]]
    assert s.tolist() == [[0.75, 0.3125, 0.0625, 1.0]]
    s, r, q = metrics_ref.reference([img], [gt], None, QUANTIZE)      # 0.5 * 255 + 0.5 = 128; 2 and -1 saturate
    f = np.float32
    assert r.tolist() == [[[[float(f(128) / f(255)), 1.0]]]] and q.tolist() == [[[[float(f(64) / f(255)), 0.0]]]]
    assert s[0, 3] == 2 and s[0, 1] == s[0, 2] and abs(float(s[0, 0]) - (64 / 255 + 1)) < 1e-7
    s = metrics_ref.reference([torch.full((2, 1, 2), float("nan"))], [torch.zeros(2, 1, 2)], [torch.zeros(1, 1, 2)], CLAMP)[0]
    assert torch.isnan(s[0, :4]).all() and s[0, 4:].tolist() == [0, 0]                 # not under the mask: not in its sum


def _views(n, C, H, W, seed, mask):
    """n views of different content on the device; values beyond [0, 1] on both sides.  mask: None, "one" ([1, H, W]),
    "full" ([C, H, W]); a fifth of the mask is exactly 0, two fifths exactly 1, the rest fractions."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=gen)                 # noqa: E731
    imgs = [1.2 * rand(C, H, W) - 0.1 for _ in range(n)]
    gts = [1.2 * rand(C, H, W) - 0.1 for _ in range(n)]
    masks = None
    if mask is not None:
        masks = []
        for _ in range(n):
            u = rand(1 if mask == "one" else C, H, W)
            masks.append(torch.where(u < 0.2, torch.zeros_like(u), torch.where(u > 0.6, torch.ones_like(u), u)))
    return imgs, gts, masks


def _check(what, got, ref, C):
    """Prints the largest relative difference of each column kind, then asserts the criteria of this file."""
    got, ref = got.cpu().numpy(), ref.numpy()
    assert got.shape == ref.shape == (len(ref), 2 * C + 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(ref == got, 0.0, np.abs(got - ref) / np.abs(ref))
    kinds = dict(abs=rel[:, :C].max(), sq=rel[:, C:2 * C].max(), masked_sq=rel[:, 2 * C].max(), count=rel[:, 2 * C + 1].max())
    print(f"{what}: max relative difference " + ", ".join(f"{k} {v:.3g}" for k, v in kinds.items()))
    assert np.array_equal(got[:, -1], ref[:, -1])
    assert rel_l2(got[:, :-1], ref[:, :-1]) < 1e-6
    assert np.all(rel <= COLUMN_TOL), kinds


@gpu
@pytest.mark.parametrize("mask", [None, "one", "full"])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_channels_masks_and_modes(C, mask):
    """37 x 61 = 2257 pixels: two workgroups per view, both with a tail."""
    from binocular3dgs_amd.evaluate import image_metrics
    n, H, W = 3, 37, 61
    imgs, gts, masks = _views(n, C, H, W, seed=10 * C + len(mask or ""), mask=mask)
    for mode in (CLAMP, QUANTIZE, CLAMP | QUANTIZE):
        got, pi, pg = image_metrics(imgs, gts, masks, mode, prepared=True)
        bare = image_metrics(imgs, gts, masks, mode)[0]
        torch.cuda.synchronize()
        ref, r, q = metrics_ref.reference(imgs, gts, masks, mode)
        differ = int((pi.cpu() != r).sum()) + int((pg.cpu() != q).sum())
        print(f"C = {C}, mask {mask}, mode {mode}: {differ} entries of the prepared pair differ")
        assert differ == 0 and torch.equal(bare, got)
        _check(f"C = {C}, mask {mask}, mode {mode}", got, ref, C)
        if mask is None:
            assert np.all(got[:, -1].cpu().numpy() == C * H * W)
        else:
            assert 0 < float(got[:, -1].min()) and float(got[:, -1].max()) < C * H * W


@gpu
@pytest.mark.parametrize("n", [31, 32, 33, 65])
def test_view_table_seam(n):
    """The kernel-argument table holds 32 views: view 32 opens a second launch with view0 = 32, view 64 a third."""
    from binocular3dgs_amd.evaluate import image_metrics
    C, H, W = 3, 7, 9
    imgs, gts, masks = _views(n, C, H, W, seed=n, mask="one")
    got, pi, pg = image_metrics(imgs, gts, masks, CLAMP, prepared=True)
    ref, r, q = metrics_ref.reference(imgs, gts, masks, CLAMP)
    assert len(torch.unique(ref[:, 0])) == n                                           # every view has its own content
    single = torch.cat([image_metrics(imgs[i:i + 1], gts[i:i + 1], masks[i:i + 1], CLAMP)[0] for i in range(n)])
    rows = (got != single).any(1).nonzero().flatten().tolist()
    print(f"{n} views: rows that differ from the single-view call {rows}; "
          f"{int((pi.cpu() != r).sum()) + int((pg.cpu() != q).sum())} entries of the prepared pair differ")
    assert rows == [] and torch.equal(pi.cpu(), r) and torch.equal(pg.cpu(), q)
    _check(f"{n} views", got, ref, C)


@gpu
@pytest.mark.parametrize("hw", [1, 255, 256, 257, 2049, 524545])
def test_pixel_counts(hw):
    """1 x N images.  A workgroup covers 256 pixels per stride and a view gets ceil(N / 2048) workgroups, 256 at most:
    524545 = 256 workgroups x 256 threads x 8 pixels + 257 is above the cap, so every workgroup strides 9 times and the
    first two a tenth time.  The mask is all ones: the count column must be C * H * W exactly."""
    from binocular3dgs_amd.evaluate import image_metrics
    n, C = 2, 3
    imgs, gts, _ = _views(n, C, 1, hw, seed=hw, mask=None)
    masks = [torch.ones(1, 1, hw, device="cuda") for _ in range(n)]
    got, pi, pg = image_metrics(imgs, gts, masks, CLAMP | QUANTIZE, prepared=True)
    ref, r, q = metrics_ref.reference(imgs, gts, masks, CLAMP | QUANTIZE)
    print(f"1 x {hw}: count {got[:, -1].tolist()}, {int((pi.cpu() != r).sum()) + int((pg.cpu() != q).sum())} prepared entries differ")
    assert got[:, -1].tolist() == [C * hw] * n
    assert torch.equal(pi.cpu(), r) and torch.equal(pg.cpu(), q)
    _check(f"1 x {hw}", got, ref, C)
    assert torch.equal(got, image_metrics(imgs, gts, None, CLAMP | QUANTIZE)[0])       # no mask = all ones


@gpu
def test_nan_pixel_under_clamp_stays_in_its_channel():
    """torch.clamp keeps a NaN and so does the kernel: one NaN pixel of channel 1 turns that channel's two sums into NaN.
    The pixel is not under the mask (mask 0 there), so the masked sum and the count do not see it; with no mask at all
    every entry counts as masked and the masked sum is NaN as well."""
    from binocular3dgs_amd.evaluate import image_metrics
    C, H, W = 3, 5, 7
    imgs, gts, masks = _views(2, C, H, W, seed=4, mask="one")
    imgs[1][1, 2, 3] = float("nan")
    masks[1][0, 2, 3] = 0.0
    got = image_metrics(imgs, gts, masks, CLAMP)[0].cpu()
    ref = metrics_ref.reference(imgs, gts, masks, CLAMP)[0]
    nan = torch.zeros(2, 2 * C + 2, dtype=torch.bool)
    nan[1, 1] = nan[1, C + 1] = True
    print(f"NaN columns of the view with the NaN pixel: {torch.isnan(got[1]).nonzero().flatten().tolist()}")
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(ref), nan)
    _check("NaN pixel, the other columns", got.masked_fill(nan, 0.0), ref.masked_fill(nan, 0.0), C)
    got = image_metrics(imgs, gts, None, CLAMP)[0].cpu()
    nan[1, 2 * C] = True
    assert torch.equal(torch.isnan(got), nan)
