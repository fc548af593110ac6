#!/usr/bin/env python
"""G15: tests/golden/cloud.npz -- the reference's matcher cloud after the matcher (submodules/dense_matcher/triangulate.py),
by IMPORTING its helpers under the CPU shim of make_golden.py and EXECUTING the script's own statements from its source text
on CPU tensors (needs the reference checkout; never runs where the tests run).  Only data leaves this script.

  scene    written here: four pinhole cameras (64x48, camera 0 at the origin with power-of-two focal lengths, so that its
           projections round the same way in any operation order), one tilted, smoothly textured plane rendered analytically
  select   the view-selection statements (lines 104-118) for a few (dataset, image count, n_views)
  pairs    per ordered view pair: matches from the known geometry plus outliers (over the 2 px threshold, out of frame, one
           exactly on the W-1 edge) -> the statements 166-170 and 174-219, with line 171-172 (cv2.triangulatePoints, not
           installed) replaced by the float64 DLT of tests/cloud_ref.py rounded to float32 as OpenCV's output is
  sheet    the DTU statements 222-238 on one view with a white region
  grow     the setup 248-262 and the loop 263-379, one execution per round, with the two in-loop counts replaced by 16 and 32:
           draws, per-candidate SSIM and mask, accepted candidates and the cloud after every round
  order    three rounds of the loop's host draws after one torch.manual_seed, for the default draw order
  window   create_window(11, 3)

Conditions asserted here so that no test hides a flip behind a tolerance: see the asserts below (margins of 1e-3 px around the
threshold, the frame bounds and the rounding boundaries; an SSIM margin d = 4 x the largest |reference fp32 - float64|).
Re-run with:  python tests/golden/make_golden_cloud.py"""
import importlib.util
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, CudaToCpu  # noqa: E402

sys.path.insert(0, os.path.dirname(OUT))
import cloud_ref  # noqa: E402

DM = os.path.join(REF, "submodules", "dense_matcher")
W, H = 64, 48
N_SEEDS, N_SAMPLES, ROUNDS = 16, 32, 12
EPS = 1e-3


def load(name):
    spec = importlib.util.spec_from_file_location("dm_" + name, os.path.join(DM, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def script_lines():
    return open(os.path.join(DM, "triangulate.py")).read().splitlines()


def block(lines, first, last, edits=()):
    """lines first..last (1-based, inclusive) of the script as a code object"""
    text = textwrap.dedent("\n".join(lines[first - 1:last]))
    for a, b in edits:
        assert a in text, a
        text = text.replace(a, b)
    return compile(text, f"triangulate.py[{first}-{last}]", "exec")


# ---- the scene ---------------------------------------------------------------------------------------------------------------
def cameras():
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 24.0], [0, 0, 1.0]])
    c2ws = [np.eye(4, dtype=np.float32)]
    for (bx, by, ax, ay) in ((7.0, 0.5, 0.01, -0.05), (-6.0, 3.0, -0.03, 0.04), (2.0, -6.0, 0.05, 0.0)):
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rt = np.eye(4)
        Rt[:3, :3] = Rx @ Ry
        Rt[:3, 3] = -Rt[:3, :3] @ np.array([bx, by, 0.0])
        c2ws.append(np.float32(np.linalg.inv(Rt)))
    return K.astype(np.float32), np.stack(c2ws)


PLANE_N, PLANE_D = np.array([-0.15, 0.05, 1.0]), 60.0             # n . X = d


def texture(X):
    x, y = X[..., 0], X[..., 1]
    ch = [0.5 + 0.45 * np.sin(0.55 * x + 0.2 * y + 0.3) * np.cos(0.15 * x - 0.5 * y),
          0.5 + 0.45 * np.sin(0.25 * x - 0.6 * y + 1.1) * np.cos(0.45 * x + 0.2 * y + 0.5),
          0.5 + 0.45 * np.cos(0.5 * x + 0.45 * y - 0.7) * np.sin(0.2 * x - 0.3 * y + 0.2)]
    return np.stack(ch, -1)


def surface_point(K, c2w, uv):
    """the plane point behind pixel coordinates uv [N,2] of a camera (float64)"""
    K, c2w = K.astype(np.float64), c2w.astype(np.float64)
    d = np.concatenate([uv, np.ones((len(uv), 1))], 1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = (PLANE_D - o @ PLANE_N) / (d @ PLANE_N)
    return o + d * t[:, None]


def render(K, c2w):
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = surface_point(K, c2w, np.stack([xs.ravel(), ys.ravel()], 1))
    return np.clip(np.round(texture(X) * 255.0), 0, 255).astype(np.uint8).reshape(H, W, 3)


def near_half(a):
    f = np.abs(a - np.floor(a) - 0.5)
    return f < EPS


# ---- pairs ---------------------------------------------------------------------------------------------------------------
def run_pair(env_base, code_p, code_t, ref_index, src_index, kp0, kp1):
    env = dict(env_base, ref_index=ref_index, src_index=src_index, mkpts0=kp0, mkpts1=kp1, points_3D=[], colors_all=[])
    env["ref_image"] = env["images"][ref_index]
    exec(code_p, env)
    P0, P1 = env["ref_p"].numpy(), env["src_p"].numpy()
    env["points"] = cloud_ref.dlt_points_f32(P0, P1, kp0, kp1)
    pin = env["points"]
    pts_in = torch.tensor(pin)
    k3 = env["intrinsic"][:3, :3]
    uv_r, _ = env["point_world2depth"](pts_in.reshape(-1, 3), k3, torch.inverse(env["extrinsics_all"][ref_index]))
    uv_s, _ = env["point_world2depth"](pts_in.reshape(-1, 3), k3, torch.inverse(env["extrinsics_all"][src_index]))
    exec(code_t, env)
    kept = env["mask"].numpy().copy()
    kept[kept] &= env["uv_mask"].numpy()
    return {"P_ref": P0, "P_src": P1, "points_in": pin,
            "uv_ref": uv_r.numpy(), "uv_src": uv_s.numpy(), "norm_ref": env["ref_norm"].numpy(), "norm_src": env["src_norm"].numpy(),
            "mask": env["mask"].numpy(), "kept": kept, "points": env["points_3D"][0], "colors_f": env["colors"],
            "colors": env["colors_all"][0], "dlt64": cloud_ref.dlt_points_f64(P0, P1, kp0, kp1)}


def pair_ok(r, exact_edge=None):
    """per match: no margin is violated"""
    thr = np.minimum(np.abs(r["norm_ref"] - 2.0), np.abs(r["norm_src"] - 2.0)) > EPS
    uv = np.concatenate([r["uv_ref"], r["uv_src"]], 1)
    hi = np.array([W - 1, H - 1, W - 1, H - 1], np.float32)
    frame = (np.abs(uv) > EPS) & (np.abs(uv - hi) > EPS)
    if exact_edge is not None:
        frame[exact_edge, 0] = True
    return thr & frame.all(1)


def make_matches(rng, K, c2ws, ref, src, n):
    """matches of the known geometry, then outliers"""
    uv = np.stack([rng.uniform(1, W - 2, n), rng.uniform(1, H - 2, n)], 1)
    X = surface_point(K, c2ws[ref], uv)
    kp0, kp1 = cloud_ref.project_f64(X, K, c2ws[ref]), cloud_ref.project_f64(X, K, c2ws[src])
    base = c2ws[src][:2, 3] - c2ws[ref][:2, 3]
    perp = np.array([-base[1], base[0]]) / np.linalg.norm(base)
    k = n // 8
    kp1[:k] += perp * rng.uniform(5.0, 12.0, (k, 1)) * rng.choice([-1, 1], (k, 1))          # far over the threshold
    kp1[k:2 * k] += perp * rng.uniform(0.3, 1.5, (k, 1))                                    # under it
    kp1[2 * k:3 * k] += perp * rng.uniform(2.5, 4.5, (k, 1))                                # around it (some in, some out)
    # consistent geometry that leaves a frame
    uv_out = np.stack([rng.uniform(-6, -0.5, k), rng.uniform(2, H - 3, k)], 1)
    uv_out[k // 2:, 0] = rng.uniform(W - 0.5, W + 5, k - k // 2)
    Xo = surface_point(K, c2ws[ref], uv_out)
    kp0 = np.concatenate([kp0, cloud_ref.project_f64(Xo, K, c2ws[ref])])
    kp1 = np.concatenate([kp1, cloud_ref.project_f64(Xo, K, c2ws[src])])
    order = rng.permutation(len(kp0))
    return kp0[order].astype(np.float32), kp1[order].astype(np.float32)


def main():
    torch.nn.Module.cuda = lambda self, *a, **k: self
    rng = np.random.default_rng(15)
    lines = script_lines()
    out = {}
    K, c2ws = cameras()
    imgs = np.stack([render(K, c) for c in c2ws])
    out["scene/K"], out["scene/c2ws"], out["scene/images"] = K, c2ws, imgs
    with CudaToCpu():
        utils = load("utils")
        ssim_mod = load("ssim")
        out["window"] = ssim_mod.create_window(11, 3)[0, 0].reshape(-1).numpy()

        # ---- select ----
        code_sel = block(lines, 104, 118)
        sel = []
        for name, n_images, n_views in (("LLFF", 4, 3), ("LLFF", 10, 3), ("LLFF", 20, 2), ("LLFF", 34, 4), ("LLFF", 61, 3), ("DTU", 49, 3),
                                        ("DTU", 49, 6)):
            import types
            env = {"np": np, "images_list": [None] * n_images,
                   "args": types.SimpleNamespace(dataset_name=name, n_views=n_views, dtu_sparse_indices=[25, 22, 28, 40, 44, 48, 0, 8, 13])}
            exec(code_sel, env)
            pairs = [(r, s) for r in env["ref_indices"] for s in env["srcs_indices"][r]]
            sel.append((name, n_images, n_views, list(env["ref_indices"]), pairs))
        out["select/cases"] = np.array([f"{a}:{b}:{c}" for a, b, c, _, _ in sel])
        for i, (_, _, _, refs, pairs) in enumerate(sel):
            out[f"select/{i}/refs"], out[f"select/{i}/pairs"] = np.array(refs), np.array(pairs)
        ref_indices, srcs_indices = sel[0][3], {r: [s for rr, s in sel[0][4] if rr == r] for r in sel[0][3]}

        # ---- pairs ----
        base = {"torch": torch, "np": np, "F": F, "point_world2depth": utils.point_world2depth,
                "extrinsics_all": torch.tensor(c2ws).float(), "intrinsics_all": torch.tensor(np.stack([K] * 4)).float(),
                "images": torch.tensor(imgs).float(), "image_w": W, "image_h": H, "image_wh": torch.tensor([W - 1, H - 1])}
        code_p, code_t = block(lines, 166, 170), block(lines, 174, 219)
        points_3D, colors_all, names = [], [], []
        for ref in ref_indices:
            for src in srcs_indices[ref]:
                kp0, kp1 = make_matches(rng, K, c2ws, ref, src, 200)
                edge = None
                if (ref, src) == (0, srcs_indices[0][0]):
                    # one match whose reference u is exactly W-1: search the float32 neighbourhood of the keypoint
                    Xe = surface_point(K, c2ws[0], np.array([[W - 1.0, 20.3]]))
                    e1 = cloud_ref.project_f64(Xe, K, c2ws[src]).astype(np.float32)
                    for k in range(-2000, 2000):
                        e0 = np.array([[W - 1.0 + k * 2.0 ** -19, 20.3]], np.float32)
                        r = run_pair(base, code_p, code_t, ref, src, e0, e1)
                        if r["uv_ref"][0, 0] == np.float32(W - 1) and r["kept"][0]:
                            kp0, kp1, edge = np.concatenate([e0, kp0]), np.concatenate([e1, kp1]), 0
                            break
                    assert edge == 0, "no keypoint lands exactly on the edge"
                r = run_pair(base, code_p, code_t, ref, src, kp0, kp1)
                ok = pair_ok(r, edge)
                # the kept points must not sit on a rounding boundary of any selected view (growth counts them per pixel)
                for v in ref_indices:
                    uv = utils.map_points_to_image(torch.tensor(r["points_in"]).reshape(-1, 1, 3), torch.inverse(base["extrinsics_all"][v])[None],
                                                   torch.tensor([K[0, 0], K[1, 1]]), torch.tensor([K[0, 2], K[1, 2]]))[0, :, 0].numpy()
                    ok &= ~(near_half(uv).any(1) & r["kept"])
                if edge is not None:
                    assert ok[0]
                kp0, kp1 = kp0[ok], kp1[ok]                              # (inputs are chosen here; the run below is what is recorded)
                r = run_pair(base, code_p, code_t, ref, src, kp0, kp1)
                assert pair_ok(r, edge).all()
                rel = np.abs(r["dlt64"] - r["points_in"]).max(1) / np.linalg.norm(r["dlt64"] - c2ws[ref][:3, 3], axis=1)
                assert rel.max() < 3e-7, rel.max()
                n, kept = len(kp0), int(r["kept"].sum())
                over, frame = int((~r["mask"]).sum()), int(r["mask"].sum()) - kept
                assert over >= 10 and frame >= 10 and kept >= 60, (over, frame, kept)
                frac = np.abs(r["colors_f"] - np.round(r["colors_f"])) < 1e-3
                assert frac.mean() < 0.01
                tag = f"pair/{ref}_{src}"
                names.append(f"{ref}_{src}")
                out[tag + "/kp_ref"], out[tag + "/kp_src"] = kp0, kp1
                for key in ("P_ref", "P_src", "kept", "points", "colors", "colors_f", "dlt64"):
                    out[tag + "/" + key] = r[key]
                print(tag, n, "matches,", kept, "kept,", over, "over the threshold,", frame, "out of frame")
                points_3D.append(r["points"])
                colors_all.append(r["colors"])
        out["pair/names"] = np.array(names)
        out["pair/edge"] = np.array([0, srcs_indices[0][0], 0])           # ref, src, row of the exact-edge match

        # ---- sheet ----
        img = imgs[1].copy()
        img[10:20, 5:30] = 255
        img[30:34, 40:50] = (254, 200, 10)
        img[36:40, 40:50] = (253, 253, 253)
        env = dict(base, args=None, ref_index=1, images=base["images"].clone(), depth2point_world=utils.depth2point_world, points_3D=[],
                   colors_all=[])
        env["images"][1] = torch.tensor(img).float()
        exec(block(lines, 222, 238), env)
        f64 = cloud_ref.sheet_points_f64(W, H, K, c2ws[1], 10.0)[env["bg_mask"]]
        err = float(np.abs(env["points_3D"][0] - f64).max())
        out["sheet/image"], out["sheet/mask"], out["sheet/points"] = img, env["bg_mask"], env["points_3D"][0]
        out["sheet/colors"], out["sheet/view"] = env["colors_all"][0], np.array(1)
        out["sheet/max_ref_err"], out["sheet/bound"] = np.array(err), np.array(4 * err)
        print("sheet:", int(env["bg_mask"].sum()), "points, reference fp32 vs float64:", err)

        # ---- grow ----
        edits = (("sample_points_num = 100", f"sample_points_num = {N_SEEDS}"), ("sample_num = 200", f"sample_num = {N_SAMPLES}"))
        code_setup, code_loop = block(lines, 248, 262), block(lines, 263, 379, edits)
        genv = dict(base, utils=utils, SSIM_v2=ssim_mod.SSIM_v2, get_projected_patch_color=utils.get_projected_patch_color,
                    map_points_to_image=utils.map_points_to_image, tqdm=lambda x: x, print=lambda *a: None, width=W, height=H,
                    points_3D=np.concatenate(points_3D, 0), colors_all=np.concatenate(colors_all, 0), ref_indices=ref_indices,
                    srcs_indices=srcs_indices)
        out["grow/start_points"], out["grow/start_colors"] = genv["points_3D"], genv["colors_all"]
        window = out["window"]
        seeds = [1000 + r for r in range(ROUNDS)]
        while True:
            env = dict(genv)
            exec(code_setup, env)
            env["iterations"] = 1
            assert env["alpha"] == 10.0 and env["ssim_threshold"] == 0.95 and env["h_patch_size"] == 5
            rec, bad, maxdiff, near = [], None, 0.0, []
            for rnd in range(ROUNDS):
                for key in ("index_selected", "ref_index_selected", "src_index_selected", "new_points", "ref_uv", "src_uv"):
                    env.pop(key, None)
                n_before = len(env["points_all"])
                torch.manual_seed(seeds[rnd])
                exec(code_loop, env)
                torch.manual_seed(seeds[rnd])                                 # the same draws again, to record them
                ref = ref_indices[torch.randperm(len(ref_indices))[0]]
                src = srcs_indices[ref][torch.randperm(len(srcs_indices[ref]))[0]]
                seed_idx = torch.randperm(len(genv["points_3D"]))[:N_SEEDS]
                noise = torch.randn(size=(N_SEEDS, N_SAMPLES, 3))
                assert ref == env["ref_idx"] and src == env["src_idx"]
                cand = env["rand_sample_points"].squeeze().numpy()
                assert np.array_equal(cand, (env["points_all"][:len(genv["points_3D"])][seed_idx][:, None, :] + noise * 10.0).reshape(-1, 3).numpy())
                mask = env["patch_mask"].reshape(-1).numpy()
                ssim = env["ssim"].reshape(-1).numpy()
                selected = env["selected"].reshape(-1).numpy()
                s64 = cloud_ref.ssim_f64(env["src_patch"].reshape(-1, 121, 3).numpy(), env["ref_patch"].reshape(-1, 121, 3).numpy(), window)
                maxdiff = max(maxdiff, float(np.abs(ssim - s64)[mask].max()) if mask.any() else 0.0)
                near.append(np.abs(ssim - 0.95)[mask].min() if mask.any() else 1.0)
                # frame margins of every candidate
                fc = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
                uvs = [utils.map_points_to_image(torch.tensor(cand).reshape(-1, 1, 3), torch.inverse(base["extrinsics_all"][v])[None],
                                                 torch.tensor(fc[:2]), torch.tensor(fc[2:]))[0, :, 0].numpy() for v in (ref, src)]
                uv4 = np.concatenate(uvs, 1)
                lim = np.array([W, H, W, H], np.float32)
                if ((np.abs(uv4) < EPS) | (np.abs(uv4 - lim) < EPS)).any():
                    bad = rnd
                accepted = np.zeros(len(cand), bool)
                # the all-ones lookup of a selected candidate: non-zero while u * W / (W - 1) - 0.5 < W (u >= 0 here)
                ixy = uv4.astype(np.float64) * (lim / (lim - 1)) - 0.5
                if (np.abs(ixy - lim) < EPS)[selected].any() or near_half(uv4[selected]).any():
                    bad = rnd
                inside = (ixy < lim).all(1)
                if "index_selected" in env:
                    idx = np.flatnonzero(selected)
                    accepted[idx[env["index_selected"].numpy()]] = True
                    assert not (accepted & ~inside).any()
                    for v in ref_indices:                                     # an appended point is counted in every view later
                        uv = utils.map_points_to_image(torch.tensor(cand[accepted]).reshape(-1, 1, 3), torch.inverse(base["extrinsics_all"][v])[None],
                                                       torch.tensor(fc[:2]), torch.tensor(fc[2:]))[0, :, 0].numpy()
                        if near_half(uv).any():
                            bad = rnd
                count_rej = int((selected & ~accepted & inside).sum())
                assert len(env["points_all"]) == n_before + int(accepted.sum())
                if bad is not None:
                    break
                rec.append({"ref": ref, "src": src, "seed_idx": seed_idx.numpy(), "noise": noise.numpy(), "ssim": ssim, "mask": mask,
                            "selected": selected, "accepted": np.flatnonzero(accepted), "length": len(env["points_all"]),
                            "count_rej": count_rej})
            d = 4 * maxdiff
            if bad is None and min(near) <= d:
                bad = int(np.argmin(near))
            if bad is None:
                break
            seeds[bad] += 100                                                     # redraw that round's noise
            print("redraw round", bad)
        live = np.concatenate([r["mask"] for r in rec])
        n_acc = sum(len(r["accepted"]) for r in rec)
        ssim_rej = sum(int((r["mask"] & ~r["selected"]).sum()) for r in rec)
        count_rej = sum(r["count_rej"] for r in rec)
        frame_rej = int((~live).sum())
        print(f"grow: live {live.mean():.2f}, accepted {n_acc}, rejected by ssim {ssim_rej}, count {count_rej}, frame {frame_rej}; "
              f"max |fp32 - f64| {maxdiff:.3g}, d {d:.3g}, nearest to the threshold {min(near):.3g}")
        assert live.mean() >= 0.25 and n_acc >= 10 and ssim_rej >= 5 and count_rej >= 5 and frame_rej >= 5
        for i, r in enumerate(rec):
            for key in ("seed_idx", "noise", "ssim", "mask", "selected", "accepted"):
                out[f"grow/{i}/{key}"] = r[key]
            out[f"grow/{i}/views"] = np.array([r["ref"], r["src"], r["length"]])
        out["grow/rounds"], out["grow/ref_indices"] = np.array(ROUNDS), np.array(ref_indices)
        out["grow/ssim_max_ref_err"], out["grow/ssim_bound"] = np.array(maxdiff), np.array(d)
        out["grow/points"], out["grow/colors_f"] = env["points_all"].numpy(), env["colors_all"].numpy()
        new = out["grow/colors_f"][len(out["grow/start_points"]):]               # (the starting colours are integers)
        assert (np.abs(new - np.round(new)) < 1e-3).mean() < 0.01

        # ---- order ----
        env = dict(genv)
        exec(code_setup, env)
        env["iterations"] = 1
        torch.manual_seed(2024)
        order = []
        for rnd in range(3):
            state = torch.get_rng_state()
            exec(code_loop, env)
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            ref = ref_indices[torch.randperm(len(ref_indices))[0]]
            src = srcs_indices[ref][torch.randperm(len(srcs_indices[ref]))[0]]
            seed_idx = torch.randperm(len(genv["points_3D"]))[:N_SEEDS]
            assert ref == env["ref_idx"] and src == env["src_idx"]
            torch.set_rng_state(after)
            order.append(np.concatenate([[ref, src], seed_idx.numpy()]))
        out["order/seed"], out["order/draws"] = np.array(2024), np.array(order)
    path = os.path.join(OUT, "cloud.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 766 * 1000


if __name__ == "__main__":
    main()
