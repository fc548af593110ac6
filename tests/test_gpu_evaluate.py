"""GPU: held-out view evaluation (binocular3dgs_amd/evaluate.py, csrc/metrics.hip).

  * b3gs_image_metrics_batch against the reference's psnr / ssim / l1_loss (golden G12): both semantics, the 8-bit round
    trip bit for bit, NaN on an empty mask, +inf on identical images, the same bits from call to call;
  * render_views against render() under no_grad, 11 views of two resolutions (crosses the 8-view launch), also from a tiny
    starting capacity (the overflow path);
  * evaluate_views / training_report against the PyTorch statements on render()'s images;
  * isolation: evaluation inside a training run changes no bit of the model, the optimiser, the densification statistics or
    the training rasterizer's buffers and words."""
import os

import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_DB = 1e-4


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))


def _dev(a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _psnr(mse):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20 * np.log10(1 / np.sqrt(mse))


def _quantise(x):
    return torch.clamp(x * 255 + 0.5, 0, 255).to(torch.uint8).to(torch.float32) / 255


def test_metrics_match_the_reference(g):
    from binocular3dgs_amd import _C
    from binocular3dgs_amd.evaluate import CLAMP, QUANTIZE, image_metrics
    imgs, gts, masks = _dev(g["img"]), _dev(g["gt"]), _dev(g["mask"])
    C, H, W = imgs[0].shape
    hw = H * W
    # semantics 1 (training_report): clamp, mean |d|, mean of the per-channel PSNRs
    s = image_metrics(imgs, gts, None, CLAMP)[0].cpu().numpy()
    l1 = s[:, :C].sum(1) / (C * hw)
    psnr = _psnr(s[:, C:2 * C] / hw).mean(1)
    assert np.all(np.abs(l1 - g["report_l1"]) <= 1e-6 * g["report_l1"])
    assert np.all(np.abs(psnr - g["report_psnr"]) <= TOL_DB)
    # semantics 2 (metrics.py): 8-bit round trip, composite with a fractional [C,H,W] mask, masked PSNR, SSIM
    s, pi, pg = image_metrics(imgs, gts, masks, QUANTIZE, prepared=True)
    s = s.cpu().numpy()
    assert torch.equal(pi.cpu(), torch.from_numpy(g["png_r"])) and torch.equal(pg.cpu(), torch.from_numpy(g["png_g"]))
    psnr = _psnr(s[:, 2 * C] / s[:, 2 * C + 1])
    assert np.all(np.abs(psnr - g["png_mask_psnr"]) <= TOL_DB), (psnr, g["png_mask_psnr"])
    l1 = s[:, :C].sum(1) / (C * hw)
    assert np.all(np.abs(l1 - g["png_mask_l1"]) <= 1e-6 * g["png_mask_l1"])
    ss = _C.ssim(pi, pg, 11, False).cpu().numpy()
    assert np.all(np.abs(ss - g["png_mask_ssim"]) <= 2e-5 * np.maximum(1.0, np.abs(g["png_mask_ssim"])))
    # LLFF: no mask (= all ones); the prepared pair is exactly the uint8 formula
    s, pi, pg = image_metrics(imgs, gts, None, QUANTIZE, prepared=True)
    s = s.cpu().numpy()
    # (on the host: to_tensor divides by 255 on the CPU; torch's device kernel multiplies by the reciprocal instead)
    assert torch.equal(pi.cpu(), _quantise(torch.stack(imgs).cpu())) and torch.equal(pg.cpu(), _quantise(torch.stack(gts).cpu()))
    assert np.all(np.abs(_psnr(s[:, 2 * C] / s[:, 2 * C + 1]) - g["png_ones_psnr"]) <= TOL_DB)
    assert np.all(s[:, 2 * C + 1] == C * hw)
    ss = _C.ssim(pi, pg, 11, False).cpu().numpy()
    assert np.all(np.abs(ss - g["png_ones_ssim"]) <= 2e-5 * np.maximum(1.0, np.abs(g["png_ones_ssim"])))
    # a [1,H,W] mask is broadcast over the channels
    m1 = [m[:1].contiguous() for m in masks]
    s1, p1, _ = image_metrics(imgs, gts, m1, QUANTIZE, prepared=True)
    s3, p3, _ = image_metrics(imgs, gts, [m[:1].expand(C, H, W).contiguous() for m in masks], QUANTIZE, prepared=True)
    assert torch.equal(s1, s3) and torch.equal(p1, p3)
    # empty mask -> NaN, identical images -> +inf (image_utils.psnr's masked branch)
    s = image_metrics(imgs[:1], gts[:1], [torch.zeros_like(masks[0])], QUANTIZE)[0].cpu().numpy()
    with np.errstate(invalid="ignore"):
        assert np.isnan(_psnr(s[0, 2 * C] / s[0, 2 * C + 1])) and np.isnan(g["psnr_empty_mask"])
    s = image_metrics(gts[:1], gts[:1], [torch.ones_like(masks[0])], QUANTIZE)[0].cpu().numpy()
    assert _psnr(s[0, 2 * C] / s[0, 2 * C + 1]) == np.inf == g["psnr_identical"]


def test_metrics_are_deterministic_and_cover_every_pixel():
    from binocular3dgs_amd.evaluate import CLAMP, image_metrics
    gen = torch.Generator(device="cuda").manual_seed(5)
    n, H, W = 9, 300, 401                            # 9 views, odd width: a tail in every workgroup's stride
    imgs = [1.2 * torch.rand(3, H, W, device="cuda", generator=gen) - 0.1 for _ in range(n)]
    gts = [torch.rand(3, H, W, device="cuda", generator=gen) for _ in range(n)]
    masks = [(torch.rand(1, H, W, device="cuda", generator=gen) > 0.3).float() for _ in range(n)]
    a, pa, ga = image_metrics(imgs, gts, masks, CLAMP, prepared=True)
    b, pb, gb = image_metrics(imgs, gts, masks, CLAMP, prepared=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(ga, gb)
    # against float64 sums by torch
    x = torch.stack(imgs).clamp(0, 1).double()
    y = torch.stack(gts).clamp(0, 1).double()
    m = torch.stack(masks).double()
    r, q = x * m + (1 - m), y * m + (1 - m)
    d = (r - q).float().double()
    ref = torch.cat([d.abs().sum((2, 3)), (d * d).sum((2, 3)), (d * d * (m == 1)).sum((1, 2, 3))[:, None],
                     (m == 1).expand_as(d).sum((1, 2, 3))[:, None].double()], 1)
    assert rel_l2(a.cpu().numpy(), ref.cpu().numpy()) < 1e-6
    assert torch.equal(a[:, -1].cpu(), ref[:, -1].cpu())


def _scene(P=20000):
    from binocular3dgs_amd import synth
    model = synth.synth_model(P, seed=11, device="cuda", width=200, height=144)
    cams = (synth.synth_cameras(200, 144, yaws=tuple(range(-16, 20, 4)), device="cuda")            # 9 views
            + synth.synth_cameras(160, 120, yaws=(3.0, -5.0), device="cuda"))                      # 2 views
    # (interleave the resolutions: the renderer groups them)
    cams = cams[:4] + cams[9:10] + cams[4:9] + cams[10:]
    bg = torch.tensor([0.1, 0.0, 0.2], device="cuda")
    return model, cams, bg


def _render_ref(model, cams, bg):
    from binocular3dgs_amd.render import PipelineParams, render
    with torch.no_grad():
        return [render(c, model, PipelineParams(), bg)["render"].clone() for c in cams]


def test_render_views_equals_render():
    from binocular3dgs_amd import evaluate
    model, cams, bg = _scene()
    ref = _render_ref(model, cams, bg)
    for capacity in (None, 1000):
        got = evaluate.render_views(model, cams, bg, capacity=capacity)
        assert len(got) == len(cams) == 11
        bitwise = True
        for a, b, c in zip(got, ref, cams):
            assert a.shape == (3, c.image_height, c.image_width)
            err = (a - b).abs()
            assert bool((err <= 2e-5 * (1 + b.abs())).all()), float(err.max())
            bitwise &= torch.equal(a, b)
        print(f"render_views vs render(): capacity={capacity} bitwise={bitwise}")
    # the tiny start grew the cached renderer (one overflow read per batch, grow, the batch again)
    caps = {k: fr.capacity for k, fr in model._b3gs_eval_renderers.items()}
    assert all(c > 1000 for c in caps.values()), caps


def test_evaluate_views_and_training_report_match_the_torch_statements():
    from binocular3dgs_amd import evaluate, loss
    model, cams, bg = _scene()
    gen = torch.Generator(device="cuda").manual_seed(2)
    for c in cams:
        c.original_image = 1.2 * torch.rand(3, c.image_height, c.image_width, device="cuda", generator=gen) - 0.1
    ref = _render_ref(model, cams, bg)
    res = evaluate.evaluate_views(model, cams, bg, mode="report")
    for v, img, c in zip(res["per_view"], ref, cams):
        a, b = img.clamp(0, 1), c.original_image.clamp(0, 1)
        assert abs(v["PSNR"] - float(loss.psnr(a, b).mean())) <= TOL_DB
        assert abs(v["L1"] - float(loss.l1_loss(a, b))) <= 1e-5 * float(loss.l1_loss(a, b))
        assert abs(v["SSIM"] - float(loss.ssim(a[None], b[None]))) <= 1e-4
    assert res["PSNR"] == float(torch.tensor([v["PSNR"] for v in res["per_view"]]).mean())
    masks = [None if i % 3 == 0 else (torch.rand(1, c.image_height, c.image_width, device="cuda", generator=gen) > 0.2).float()
             for i, c in enumerate(cams)]
    res = evaluate.evaluate_views(model, cams, bg, mode="png", masks=masks)
    for v, img, c, m in zip(res["per_view"], ref, cams, masks):
        m = torch.ones_like(img[:1]) if m is None else m
        r, q = _quantise(img) * m + (1 - m), _quantise(c.original_image) * m + (1 - m)
        d = (r - q)[(m == 1).expand_as(r)]
        assert abs(v["PSNR"] - float(20 * torch.log10(1 / torch.sqrt((d * d).mean())))) <= TOL_DB
        assert abs(v["SSIM"] - float(loss.ssim(r[None], q[None]))) <= 1e-4
    # training_report: device sums against render() + the PyTorch statements, float64 averaging
    test, train = cams[:4], cams[4:7]
    got = evaluate.training_report(model, test, train, bg)

    def stmts(image, gt):
        return loss.l1_loss(image, gt).mean().double(), loss.psnr(image, gt).mean().double()
    want = evaluate.training_report(model, test, train, bg, render_fn=lambda cs: _render_ref(model, cs, bg),
                                    view_metrics=stmts)
    assert list(got) == list(want) == ["test", "train"]
    for k in got:
        assert abs(got[k][0] - want[k][0]) <= 1e-5 * want[k][0] and abs(got[k][1] - want[k][1]) <= TOL_DB


def _train_state(model, opt, fr):
    st = [p.detach().clone() for p in model.parameters()]
    st += [opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._step_words.clone(), model.denom.clone(),
           model.xyz_gradient_accum.clone(), model.max_radii2D.clone()]
    for s in fr.slots:                    # open-tile prediction and repair counters live in the image buffers
        st += [s.img.clone(), s.radii.clone(), s.color.clone()]
    st += [fr.high_water.clone(), fr.overflow_flag.clone(), fr._n_all.clone()]
    return st, (fr.capacity, fr.seg1_fraction, fr.depth_key_bits, fr.P)


def test_evaluation_leaves_training_state_alone():
    from binocular3dgs_amd import evaluate, synth
    from binocular3dgs_amd.fused import FusedRasterizer
    from binocular3dgs_amd.step import FusedAdam, ViewShardedStep
    W, H = 160, 120
    gc, gd, ga = synth.synth_pixel_grads(W, H, seed=1, device="cuda")
    fn = lambda i, pkg, spkg: [(pkg["render"], gc), (pkg["rendered_depth"], gd), (pkg["rendered_alpha"], ga), (spkg["render"], gc)]  # noqa: E731
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 0.05]
    finals = []
    for with_eval in (False, False, True):
        model = synth.synth_model(9000, seed=7, device="cuda", width=W, height=H)
        pairs = synth.synth_view_set(W, H, device="cuda")
        bg = torch.tensor([0.1, 0.0, 0.2], device="cuda")
        model.init_densification_stats()
        opt = FusedAdam(model.parameters(), lrs, eps=1e-15)
        fr = FusedRasterizer(model, W, H, num_slots=2 * len(pairs), want_means2D=False)
        st = ViewShardedStep(model, pairs, bg, optimizer=opt, fused=fr)
        test = synth.synth_cameras(W, H, yaws=(2.0, -3.0, 7.0, 11.0, -9.0), device="cuda")
        for c in test:
            c.original_image = torch.rand(3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(c.uid))
        for it in range(1, 21):
            st.step(pair_grad_fn=fn)
            if with_eval and it % 5 == 0:
                torch.cuda.synchronize()
                before, words = _train_state(model, opt, fr)
                res = evaluate.evaluate_views(model, test, bg, mode="report")
                evaluate.evaluate_views(model, test[:2], bg, mode="png")
                assert np.isfinite(res["PSNR"])
                torch.cuda.synchronize()
                after, words2 = _train_state(model, opt, fr)
                assert words == words2
                for k, (x, y) in enumerate(zip(before, after)):
                    assert torch.equal(x, y), f"evaluation changed training state entry {k} at step {it}"
        torch.cuda.synchronize()
        finals.append(_train_state(model, opt, fr)[0][:12])
    repeat = all(torch.equal(x, y) for x, y in zip(finals[0], finals[1]))
    bitwise = all(torch.equal(x, y) for x, y in zip(finals[0], finals[2]))
    print(f"20 steps: run repeated bitwise={repeat}; with / without evaluation bitwise={bitwise}")
    if repeat:
        assert bitwise, "the run with evaluation differs from two identical runs without it"
    # (otherwise the chain rule's float atomics already make two runs without evaluation differ in the last bits)
    for x, y in zip(finals[0], finals[2]):
        assert rel_l2(x.double().cpu().numpy(), y.double().cpu().numpy()) < 1e-5
