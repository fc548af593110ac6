"""GPU: per-Gaussian gradient parity of the projection backward (csrc/preprocess.hip gaussian_backward: standard backward,
and the fused multi-view step on raw parameters) with float64 autograd of oracle/dense_torch.py, at the branches no other
test reaches with an independent reference: the frustum clamp of the EWA Jacobian (x, y, both), SH degrees 2 and 3 (also an
active degree below the stored one), colour channels clamped at 0 (one, two, three), non-unit quaternions.

Scene: helpers.edge_scene (P = 768, 80 x 48 = 5 x 3 tiles).  The integer tile rects of the HIP forward are imposed on the
reference; pixels whose decisions are fragile in the reference get no upstream gradient (helpers.FRAGILE_MARGIN).

Criteria: images 3e-5 (1 + |x|); per tensor relative L2 <= 2e-4, whole scene and within each stratum; per row
helpers.row_err <= ROW_BOUND for all but 0.5 % of the touched rows (2 % of a stratum's).  ROW_BOUND = 1.5e-4 is ten times the
largest 99th percentile of the REFERENCE in float32 against itself in float64 (1.56e-5 over all configurations used here;
per tensor at (K, degree) = (16, 3), 99th percentile / maximum: means3D 8.9e-6 / 4.1e-5 and 1.1e-5 / 7.7e-5 for seeds 0 and
1, opacities 7.7e-6 / 1.7e-5 and 1.1e-5 / 3.1e-5, scales 9.7e-6 / 2.2e-5 and 6.7e-6 / 1.8e-5, rotations 7.1e-6 / 2.8e-5 and
8.0e-6 / 2.1e-5, shs 5.0e-6 / 9.4e-6 and 4.9e-6 / 8.5e-6, means2D 1.0e-5 / 3.8e-5 and 1.3e-5 / 7.1e-5; table and reasoning
next to helpers.row_err).  tests/test_oracle.py (ka12) shows that criterion failing four wrong chain rules.

Populations (touched = the reference's opacity gradient is non-zero; reference side, tile rects of oracle/tile_ref.c):
  standard, scale_modifier 0.8, (K, degree) = (16, 3):
    seed 0: 713 touched; clamped in x only 64, y only 61, both 59; one / two / three channels clamped 211 / 68 / 8
    seed 1: 725 touched; clamped in x only 63, y only 63, both 60; one / two / three channels clamped 233 / 73 / 14
    (degree 0: 109 / 34 / 9 and 120 / 42 / 3 channels clamped; every test asserts >= 20 per stratum, >= 3 for three channels)
  fused, modifier 1, the yaw-8 camera of synth_view_set and its binocular partner, stratum A placed for both in turn, degree 3:
    seed 0: camera 0: 708 touched, 64 / 64 / 64 clamped, 210 / 71 / 8 channels; camera 1: 706, 64 / 65 / 63, 209 / 68 / 9
    seed 1: camera 0: 717 touched, 63 / 67 / 61 clamped, 239 / 66 / 10 channels; camera 1: 719, 66 / 67 / 61, 239 / 67 / 12
"""
import numpy as np
import pytest
import torch

from helpers import (STRATA, dense_grads, edge_scene, edge_strata, rel_l2, robust_pixel_grads, row_err, row_failures,
                     strata_population)

pytestmark = pytest.mark.gpu


def _pixel_grads(W, H, seed):
    g = torch.Generator().manual_seed(500 + seed)
    return tuple(torch.randn(c, H, W, generator=g, dtype=torch.float64) for c in (3, 1, 1))


def _hip_rect(radii, records, W, H):
    """The tile rect of every Gaussian, derived from the HIP forward's radius and pixel position exactly as the kernel does."""
    rad = radii.float()
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cl = lambda v, hi: torch.clamp(v, 0, hi).to(torch.int64)  # noqa: E731
    rect = torch.stack([cl((records[:, 0] - rad) / 16, gx), cl((records[:, 1] - rad) / 16, gy),
                        cl((records[:, 0] + rad + 15) / 16, gx), cl((records[:, 1] + rad + 15) / 16, gy)], 1)
    rect[radii <= 0] = 0
    return rect


def _check_gradients(got, ref, touched, strata, names=STRATA, label=""):
    """Per-tensor and per-row criteria, whole scene and per stratum.  Every figure is printed before anything is asserted."""
    bad = []
    for k, r in ref.items():
        g = np.asarray(got[k], dtype=np.float64).reshape(r.shape)
        e = row_err(g, r, touched)
        l2 = rel_l2(g, r)
        print(f"{label} {k}: rel L2 {l2:.2e}; row_err p50 {np.percentile(e, 50):.1e} p99 {np.percentile(e, 99):.1e} "
              f"max {e.max():.1e}")
        if l2 > 2e-4:
            bad.append((k, "rel L2", l2))
        for s in names:
            m = strata[s] & touched
            if np.abs(r[m]).max(initial=0.0) > 0:
                l2s = rel_l2(g[m], r[m])
                if l2s > 2e-4:
                    bad.append((k, s, "rel L2", l2s))
        bad += [(k,) + f for f in row_failures(g, r, touched, strata, names=names)]
    assert bad == [], f"{label}: {bad}"


@pytest.mark.parametrize("K,deg,mode", [(16, 0, "sh_sr"), (16, 1, "sh_sr"), (16, 2, "sh_sr"), (16, 3, "sh_sr"), (9, 2, "sh_sr"),
                                        (16, 3, "sh_cov")])
@pytest.mark.parametrize("seed", [0, 1])
def test_standard_backward_vs_dense_autograd_per_gaussian(seed, K, deg, mode):
    from binocular3dgs_amd import _C
    from binocular3dgs_amd.gaussian_model import covariance_from_scaling_rotation
    from test_gpu_parity import _run_hip_forward
    d, _, _ = edge_scene(seed=seed, K=K, sh_degree=deg)
    P, W, H, mod = d["means3D"].shape[0], d["W"], d["H"], d["scale_modifier"]
    if mode == "sh_cov":
        d["cov3D_precomp"] = covariance_from_scaling_rotation(d["scales"], mod, torch.nn.functional.normalize(d["rotations"]))
    out = _run_hip_forward(d, mode)
    radii = out["radii"].cpu()
    rect = _hip_rect(radii, out["views"]["records"].cpu(), W, H)
    names = ("means3D", "opacities", "shs") + (("cov3D_precomp",) if mode == "sh_cov" else ("scales", "rotations"))
    dd = {k: v for k, v in d.items() if mode != "sh_cov" or k not in ("scales", "rotations")}
    ref_out, ref, (gc, gd, ga) = dense_grads(dd, rect, _pixel_grads(W, H, seed), names=names)
    # (radii reach 150 px here: ceil() of a float32 and of a float64 value may differ by one; the rects are imposed anyway)
    assert int((ref_out["radii"] - radii).abs().max()) <= 1 and float((ref_out["radii"] != radii).float().mean()) < 0.01
    for k in ("color", "depth", "alpha"):
        r = ref_out[k].numpy()
        err = np.abs(out[k].cpu().numpy() - r) / (1 + np.abs(r))
        assert err.max() < 3e-5, (k, float(err.max()))
    touched = ref["opacities"][:, 0] != 0
    strata = edge_strata(d)
    print(f"seed {seed} K {K} degree {deg} {mode}: touched {int(touched.sum())} {strata_population(strata, touched)}")
    G, sh, colors, scales, rots, cov = out["inputs"]
    res = _C.rasterize_gaussians_backward(
        G["bg"], G["means3D"], out["radii"], colors, scales, rots, mod, cov, G["viewmatrix"], G["projmatrix"],
        d["tanfovx"], d["tanfovy"], gc.float().cuda(), gd.float().cuda(), ga.float().cuda(), sh, deg,
        G["campos"], out["geom"], out["n"], out["binning"], out["img"], out["alpha"], False)
    hip = {k: v.cpu() for k, v in zip(("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
                                       "dL_dscales", "dL_drotations"), res)}
    got = {"means3D": hip["dL_dmeans3D"], "opacities": hip["dL_dopacity"], "shs": hip["dL_dsh"].reshape(P, -1),
           "means2D": hip["dL_dmeans2D"][:, :2]}
    if mode == "sh_cov":
        got["cov3D_precomp"] = hip["dL_dcov3D"]
    else:
        got["scales"], got["rotations"] = hip["dL_dscales"], hip["dL_drotations"]
    got = {k: v.numpy() for k, v in got.items()}
    _check_gradients(got, ref, touched, strata, label=f"seed {seed} K {K} degree {deg} {mode}")
    # exact zeros: SH rows above the active degree, every entry of a clamped channel (channels the reference clamps by
    # more than float32 can get wrong), every gradient of a culled Gaussian
    dsh = hip["dL_dsh"].numpy().reshape(P, K, 3)
    assert float(np.abs(dsh[:, (deg + 1) ** 2:]).max(initial=0.0)) == 0.0
    clamped = strata["colour"] < -1e-4
    assert int(clamped.sum()) > 100 and float(np.abs(dsh.transpose(0, 2, 1)[clamped]).max()) == 0.0
    culled = (radii <= 0).numpy()
    assert culled.any()
    for k, v in got.items():
        assert float(np.abs(v[culled]).max()) == 0.0, k


@pytest.mark.parametrize("active", [2, 3])
@pytest.mark.parametrize("seed", [0, 1])
def test_fused_raw_backward_vs_autograd_through_the_activations(seed, active):
    """The fused multi-view step (FusedRasterizer: raw parameters in, activations and their chain rule in-kernel, two views
    into the same gradients) against render_dense on exp / normalize / sigmoid of float64 leaves, summed over the views."""
    from oracle import dense_torch
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.debug import state_views
    from binocular3dgs_amd.fused import FusedRasterizer
    from binocular3dgs_amd.gaussian_model import GaussianModel, inverse_sigmoid
    W, H, K = 80, 48, 16
    pair = synth.synth_view_set(W, H)[1]
    cpu_cams = [pair[0], pair[1]]
    d, _, _ = edge_scene(W=W, H=H, seed=seed, K=K, sh_degree=active, place_cams=cpu_cams)
    P = d["means3D"].shape[0]
    raw = dict(xyz=d["means3D"], f_dc=d["shs"][:, :1].contiguous(), f_rest=d["shs"][:, 1:].contiguous(),
               scaling=torch.log(d["scales"]), rotation=d["rotations"], opacity=inverse_sigmoid(d["opacities"]).reshape(P, 1))
    model = GaussianModel.from_tensors(raw["xyz"], raw["f_dc"], raw["f_rest"], raw["scaling"], raw["rotation"],
                                       raw["opacity"], sh_degree=3, active_sh_degree=active, device="cuda")
    gpair = synth.synth_view_set(W, H, device="cuda")[1]
    cams = [gpair[0], gpair[1]]
    bg = d["bg"].cuda()
    fr = FusedRasterizer(model, W, H, num_slots=2)
    outs = fr.render_batch([(cams[0], 0), (cams[1], 1)], bg)
    torch.cuda.synchronize()
    assert not fr.overflowed()

    # reference: float64 leaves of the raw parameters, the HIP rects of each view imposed
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in raw.items()}
    act = dict(means3D=leaf["xyz"], shs=torch.cat([leaf["f_dc"], leaf["f_rest"]], 1), scales=torch.exp(leaf["scaling"]),
               rotations=torch.nn.functional.normalize(leaf["rotation"]), opacities=torch.sigmoid(leaf["opacity"]))
    ref = {k: np.zeros((P, v[0].numel())) for k, v in raw.items()}
    flat_o, flat_g, per_view = [], [], []
    for v, (cam, o) in enumerate(zip(cpu_cams, outs)):
        sl = fr.slots[v]
        radii = o["radii"].cpu()
        rec = state_views(P, W, H, fr.capacity, sl.geom, sl.binning, sl.img)["records"].cpu()
        rect = _hip_rect(radii, rec, W, H)
        off = torch.zeros(P, 2, dtype=torch.float64, requires_grad=True)
        r = dense_torch.render_dense(**act, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                                     campos=cam.camera_center, bg=d["bg"], W=W, H=H, tanfovx=d["tanfovx"], tanfovy=d["tanfovy"],
                                     sh_degree=active, scale_modifier=1.0, rect=rect, pix_offset=off)
        for k, hk, scale in (("color", "render", 1.0), ("depth", "rendered_depth", 1.0), ("alpha", "rendered_alpha", 1.0)):
            x = r[k].detach().numpy()
            err = np.abs(o[hk].detach().cpu().numpy() - x) / (1 + np.abs(x))
            assert err.max() < 3e-5, (v, k, float(err.max()))
        gc, gd, ga = robust_pixel_grads({"margin": r["margin"]}, _pixel_grads(W, H, seed + 10 * v))
        for t in leaf.values():
            t.grad = None
        ((r["color"] * gc).sum() + (r["depth"] * gd).sum() + (r["alpha"] * ga).sum()).backward(retain_graph=True)
        view = {k: t.grad.reshape(P, -1).numpy().copy() for k, t in leaf.items()}
        for k in ref:
            ref[k] += view[k]
        touched = view["opacity"][:, 0] != 0
        dv = dict(d, viewmatrix=cam.world_view_transform, campos=cam.camera_center)
        strata = edge_strata(dv, sh_degree=active)
        print(f"seed {seed} active degree {active} camera {v}: touched {int(touched.sum())} {strata_population(strata, touched)}")
        per_view.append((touched, strata, off.grad.numpy() * np.array([0.5 * W, 0.5 * H])))
        flat_o += [o["render"], o["rendered_depth"], o["rendered_alpha"]]
        flat_g += [gc.float().cuda(), gd.float().cuda(), ga.float().cuda()]
    torch.autograd.backward(flat_o, flat_g)
    torch.cuda.synchronize()
    got = {k: p.grad.cpu().numpy().reshape(P, -1) for k, p in zip(("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity"),
                                                                  model.parameters())}
    # a Gaussian is in a stratum of the summed gradient when it is in it, and touched, for one of the cameras
    touched = per_view[0][0] | per_view[1][0]
    strata = {f"{s}@{v}": per_view[v][1][s] & per_view[v][0] for v in (0, 1) for s in STRATA}
    _check_gradients(got, ref, touched, strata, names=tuple(strata), label=f"seed {seed} active degree {active}")
    for v, (t, s, m2d) in enumerate(per_view):
        _check_gradients({"means2D": outs[v]["viewspace_points_grad"][:, :2].cpu().numpy()}, {"means2D": m2d}, t, s,
                         label=f"seed {seed} active degree {active} camera {v}")
    assert float(np.abs(got["f_rest"].reshape(P, K - 1, 3)[:, (active + 1) ** 2 - 1:]).max(initial=0.0)) == 0.0
    for sl in fr.slots:
        assert float(sl.scratch.abs().max()) == 0.0
