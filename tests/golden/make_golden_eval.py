#!/usr/bin/env python
"""G12: tests/golden/eval_metrics.npz -- the reference's evaluation numbers, by IMPORTING its Python under the CPU shim of
make_golden.py and calling it on seeded render / gt pairs:

    utils/image_utils.py:18-24   psnr(image, gt) on [3,H,W] (unmasked: mean of per-channel PSNRs after .mean());
                                 psnr(r, g, mask=m[None]) on [1,3,H,W] (masked branch of metrics.py:105)
    utils/loss_utils.py:36-66    ssim(r[None], g[None])                          (metrics.py:104)
    utils/loss_utils.py:18-21    l1_loss(image, gt)                              (train.py:246)
    train.py:226-261             training_report itself, with a stand-in scene / render function: the printed L1 and PSNR
                                 of both configs (3 train views -> cameras 2,1,0,2,1), and of a run without test views

The PNG round trip of render.py / metrics.py (torchvision's save_image + to_tensor, not installed here) is restated as
uint8(clamp(x*255 + 0.5, 0, 255)) / 255.  Pairs hold values outside [0,1] and values within an ulp of k/255 and of
(k - 0.5)/255 (where the round trip changes bucket); masks are fractional with exact 0 and 1 regions.
Only data leaves this script.  Re-run with:  python tests/golden/make_golden_eval.py"""
import io
import os
import re
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, CudaToCpu, install_shim  # noqa: E402

NV, C, H, W = 3, 3, 24, 32


def quantise(x):
    return torch.clamp(x * 255 + 0.5, 0, 255).to(torch.uint8).to(torch.float32) / 255


def pairs(g):
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    img = 1.4 * r(NV, C, H, W) - 0.2                       # ~28 % outside [0,1]
    gt = (img + 0.3 * (r(NV, C, H, W) - 0.5)).clamp(-0.05, 1.05)
    # every 7th element: within an ulp of a bucket edge of the 8-bit round trip
    k = torch.randint(0, 256, (NV, C, H, W), generator=g).float()
    edge = torch.where(r(NV, C, H, W) < 0.5, k / 255, (k - 0.5) / 255)
    ulp = torch.randint(-1, 2, (NV, C, H, W), generator=g)
    edge = torch.nextafter(edge, torch.where(ulp > 0, torch.ones_like(edge), -torch.ones_like(edge)))
    edge = torch.where(ulp == 0, (torch.where(r(NV, C, H, W) < 0.5, k / 255, (k - 0.5) / 255)), edge)
    sel = (torch.arange(NV * C * H * W).view(NV, C, H, W) % 7) == 0
    img = torch.where(sel, edge, img)
    gt = torch.where(sel.roll(3, -1), edge.roll(5, -1), gt)
    u = r(NV, 1, H, W)
    mask = torch.where(u < 0.55, torch.ones_like(u), torch.where(u > 0.85, torch.zeros_like(u), r(NV, 1, H, W)))
    mask = mask.expand(NV, C, H, W).contiguous()
    mask[:, 1, :2] = 0.5                                   # channels differ in a few rows: [C,H,W] masks are per element
    return img.contiguous(), gt.contiguous(), mask


def main():
    install_shim({})
    torch.nn.Module.cuda = lambda self, *a, **k: self
    g = torch.Generator().manual_seed(424242)
    out = {}
    with CudaToCpu():
        import train                                          # the reference's train.py (read-only import)
        from utils.image_utils import psnr
        from utils.loss_utils import l1_loss, ssim
        img, gt, mask = pairs(g)
        out.update(img=img.numpy(), gt=gt.numpy(), mask=mask.numpy())

        # ---- semantics 1: training_report's per-view statements --------------------------------------------------------
        rep_l1, rep_psnr = [], []
        for v in range(NV):
            a, b = torch.clamp(img[v], 0.0, 1.0), torch.clamp(gt[v], 0.0, 1.0)
            rep_l1.append(l1_loss(a, b).mean().double().item())
            rep_psnr.append(psnr(a, b).mean().double().item())
        out.update(report_l1=np.array(rep_l1), report_psnr=np.array(rep_psnr))

        # ---- semantics 2: metrics.py over the PNG round trip, masked and unmasked --------------------------------------
        for tag, mk in (("png_mask", mask), ("png_ones", torch.ones_like(mask))):
            q_img, q_gt = quantise(img), quantise(gt)
            ps, ss, l1s, rr, gg = [], [], [], [], []
            for v in range(NV):
                m = mk[v]
                rv = q_img[v] * m + (1 - m)
                gv = q_gt[v] * m + (1 - m)
                rr.append(rv)
                gg.append(gv)
                ps.append(psnr(rv[None], gv[None], mask=m[None]).item())
                ss.append(ssim(rv[None], gv[None]).item())
                l1s.append(l1_loss(rv, gv).item())
            out.update({f"{tag}_psnr": np.array(ps, np.float32), f"{tag}_ssim": np.array(ss, np.float32),
                        f"{tag}_l1": np.array(l1s, np.float32)})
            if tag == "png_mask":
                out.update(png_r=torch.stack(rr).numpy(), png_g=torch.stack(gg).numpy())
        z = torch.zeros(1, C, H, W)
        out["psnr_empty_mask"] = np.float32(psnr(img[:1], gt[:1], mask=z).item())          # nan
        out["psnr_identical"] = np.float32(psnr(gt[:1], gt[:1], mask=torch.ones_like(z)).item())   # +inf

        # ---- training_report itself: stand-in scene and render function ------------------------------------------------
        class View:
            def __init__(self, uid, image, render):
                self.uid, self.original_image, self.image_name = uid, image, f"{uid:05d}"
                self._render = render

        class Scene:
            def __init__(self, train_views, test_views):
                self.tr, self.te, self.gaussians = train_views, test_views, None

            def getTrainCameras(self):
                return self.tr

            def getTestCameras(self):
                return self.te

        r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
        nt, ne = 3, 2
        tr_img, tr_gt = 1.3 * r(nt, C, H, W) - 0.15, 1.2 * r(nt, C, H, W) - 0.1
        te_img, te_gt = 1.3 * r(ne, C, H, W) - 0.15, 1.2 * r(ne, C, H, W) - 0.1
        out.update(rep_train_img=tr_img.numpy(), rep_train_gt=tr_gt.numpy(), rep_test_img=te_img.numpy(),
                   rep_test_gt=te_gt.numpy())
        train_views = [View(i, tr_gt[i], tr_img[i]) for i in range(nt)]
        test_views = [View(100 + i, te_gt[i], te_img[i]) for i in range(ne)]
        render_fn = lambda view, gaussians, *args: {"render": view._render}  # noqa: E731
        pat = re.compile(r"Evaluating (\w+): L1 (\S+) PSNR (\S+)")       # 0-d tensors format as python floats: repr digits
        for run, tests in (("full", test_views), ("no_test", [])):
            buf = io.StringIO()
            with redirect_stdout(buf):
                train.training_report(None, 7000, None, None, l1_loss, 0.0, [7000], Scene(train_views, tests), render_fn,
                                      (None, None))
            found = pat.findall(buf.getvalue().replace("\n", " "))
            assert found, buf.getvalue()
            for name, l1v, psv in found:
                out[f"tr_{run}_{name}"] = np.array([float(l1v), float(psv)], dtype=np.float64)
            out[f"tr_{run}_configs"] = np.array([name for name, _, _ in found])
    path = os.path.join(OUT, "eval_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {sorted(out)}")


if __name__ == "__main__":
    main()
