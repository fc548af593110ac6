#!/usr/bin/env python
"""G14: tests/golden/scene_prep.npz and the tiny dataset folders scene_llff/, scene_llff_txt/, scene_dtu/scan5/, scene_blender/
-- the reference's dataset loading, by IMPORTING its Python under the CPU shim of make_golden.py (needs the reference checkout
and Pillow; never runs where the tests run):

  folders  written by this script's own writers: COLMAP cameras / images / points3D as .bin (scene_llff: 10 cameras, one of
           them SIMPLE_PINHOLE, 32x24 PNGs, a poses_bounds.npy; scene_dtu/scan5: 49 cameras, 8x6 PNGs) and as .txt
           (scene_llff_txt, PINHOLE only: the reference's text reader accepts nothing else), Blender transforms_train / _test
           with 8x6 RGBA PNGs
  (a) prep seeded uint8 sources (RGB, RGBA with alpha 0 / 255 / other, gray; shrinking by 8, 2, a non-integer factor,
           enlarging, one or both axes unchanged; a DTU-like image with a dark border holding 14/15/16/29/30/31 and dark runs
           shorter and longer than 50 rows) through the reference's loadCam (PILtoTorch, the composite, Camera) for both
           white_background values, and through the DTU statements of train.py (executed from its source text on the CPU
           tensors) for both thresholds; the output sizes loadCam picks for resolutions -1, 1, 2, 4, 8, 300
  (b) scenes readColmapSceneInfo (bin and txt, LLFF and DTU splits, n_views 3 and 0) and readNerfSyntheticInfo on the folders:
           names in order, R, T, FoVs, sizes, split membership, radius, translate, ply_path, camera_to_JSON entries; and
           loadCam's ground truth of the scene_llff / scene_blender views at resolution 2

Only data leaves this script.  Re-run with:  python tests/golden/make_golden_scene.py"""
import json
import os
import struct
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, CudaToCpu, install_shim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)

RESOLUTIONS = (-1, 1, 2, 4, 8, 300)
# name, (Ws, Hs), channels, output (w, h)
PREP = (("rgb_by8", (161, 120), 3, (20, 15)), ("rgba_frac", (121, 90), 4, (73, 60)), ("rgba_by2", (96, 128), 4, (48, 64)),
        ("rgb_up", (64, 48), 3, (100, 75)), ("rgba_w_same", (64, 48), 4, (64, 30)), ("rgba_h_same", (64, 48), 4, (40, 48)),
        ("rgba_same", (64, 48), 4, (64, 48)), ("gray_by2", (50, 40), 1, (25, 20)), ("dtu_same", (40, 160), 3, (40, 160)),
        ("dtu_by2", (80, 240), 3, (40, 120)))


# ---- writers ---------------------------------------------------------------------------------------------------------------
def png(path, a):
    from binocular3dgs_amd.frames import _chunk
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else a.shape[2]
    rows = np.zeros((H, 1 + C * W), dtype=np.uint8)
    rows[:, 1:] = a.reshape(H, C * W)
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {1: 0, 2: 4, 3: 2, 4: 6}[C], 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 9)) + _chunk(b"IEND", b""))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fp:
        fp.write(data)


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def rig(rng, n, spread):
    """n poses looking roughly down +z from a jittered grid: [(qvec, tvec)]"""
    out = []
    for k in range(n):
        ax, ay, az = rng.uniform(-0.1, 0.1, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        q = rot_to_quat(Rx @ Ry @ Rz)
        t = np.array([spread * (k % 5 - 2), spread * (k // 5 - 1), 0.0]) + rng.normal(0, 0.05, 3)
        out.append((q / np.linalg.norm(q), t))
    return out


def write_colmap(folder, cams, images, points, text):
    """cams: [(id, model id, w, h, params)], images: [(id, q, t, cam id, name)], points: (xyz, rgb)"""
    sp = os.path.join(folder, "sparse", "0")
    os.makedirs(sp, exist_ok=True)
    names = {0: "SIMPLE_PINHOLE", 1: "PINHOLE"}
    if text:
        with open(os.path.join(sp, "cameras.txt"), "w") as fp:
            fp.write("# Camera list\n")
            for cid, model, w, h, params in cams:
                fp.write(f"{cid} {names[model]} {w} {h} " + " ".join(repr(float(p)) for p in params) + "\n")
        with open(os.path.join(sp, "images.txt"), "w") as fp:
            fp.write("# Image list\n")
            for iid, q, t, cid, name in images:
                fp.write(f"{iid} " + " ".join(repr(float(v)) for v in list(q) + list(t)) + f" {cid} {name}\n")
                fp.write("1.5 2.5 -1\n")
        with open(os.path.join(sp, "points3D.txt"), "w") as fp:
            fp.write("# 3D point list\n")
            for i, (p, c) in enumerate(zip(*points)):
                fp.write(f"{i + 1} " + " ".join(repr(float(v)) for v in p) + " " + " ".join(str(int(v)) for v in c) + " 0.5 1 0\n")
        return
    with open(os.path.join(sp, "cameras.bin"), "wb") as fp:
        fp.write(struct.pack("<Q", len(cams)))
        for cid, model, w, h, params in cams:
            fp.write(struct.pack("<iiQQ", cid, model, w, h) + struct.pack("<" + "d" * len(params), *params))
    with open(os.path.join(sp, "images.bin"), "wb") as fp:
        fp.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name in images:
            fp.write(struct.pack("<idddddddi", iid, *q, *t, cid) + name.encode() + b"\x00")
            fp.write(struct.pack("<Q", 1) + struct.pack("<ddq", 1.5, 2.5, -1))
    with open(os.path.join(sp, "points3D.bin"), "wb") as fp:
        fp.write(struct.pack("<Q", len(points[0])))
        for i, (p, c) in enumerate(zip(*points)):
            fp.write(struct.pack("<QdddBBBd", i + 1, *p, *[int(v) for v in c], 0.5) + struct.pack("<Q", 1) + struct.pack("<ii", 1, 0))


def smooth_image(rng, H, W, C):
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    a = np.stack([127 + 120 * np.sin(2 * np.pi * (rng.uniform(0.5, 2) * xx + rng.uniform(0.5, 2) * yy + rng.uniform()))
                  for _ in range(C)], -1)
    return np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)


def make_folders(rng):
    pts = (rng.normal(0, 0.6, (300, 3)) + np.array([0, 0, 4.0]), rng.integers(0, 256, (300, 3)))
    # LLFF, binary: camera 2 is SIMPLE_PINHOLE; names out of order in the file
    poses = rig(rng, 10, 0.3)
    cams = [(1, 1, 32, 24, (30.0, 31.0, 16.0, 12.0)), (2, 0, 32, 24, (29.5, 16.0, 12.0))]
    order = [3, 0, 7, 1, 9, 4, 2, 8, 5, 6]
    images = [(k + 1, poses[i][0], poses[i][1], 2 if i == 4 else 1, f"IMG_{i:03d}.png") for k, i in enumerate(order)]
    llff = os.path.join(OUT, "scene_llff")
    write_colmap(llff, cams, images, pts, text=False)
    for i in range(10):
        png(os.path.join(llff, "images", f"IMG_{i:03d}.png"), smooth_image(rng, 24, 32, 3))
    pb = []
    for q, t in poses:                                      # poses_bounds.npy (spiral paths): c2w in LLFF's axis order
        from binocular3dgs_amd.dataset_readers import quaternion_to_rotation
        R = quaternion_to_rotation(q)
        c2w = np.concatenate([R.T, (-R.T @ t)[:, None]], 1)
        blk = np.concatenate([np.stack([c2w[:, 1], c2w[:, 0], -c2w[:, 2], c2w[:, 3]], 1), np.array([[24.0], [32.0], [30.0]])], 1)
        pb.append(np.concatenate([blk.ravel(), [2.0, 8.0]]))
    np.save(os.path.join(llff, "poses_bounds.npy"), np.array(pb))
    # LLFF, text
    txt = os.path.join(OUT, "scene_llff_txt")
    write_colmap(txt, [(1, 1, 8, 6, (9.0, 9.5, 4.0, 3.0))], [(k + 1, poses[i][0], poses[i][1], 1, f"v{i}.png")
                                                             for k, i in enumerate(order)], (pts[0][:20], pts[1][:20]), text=True)
    for i in range(10):
        png(os.path.join(txt, "images", f"v{i}.png"), smooth_image(rng, 6, 8, 3))
    # DTU: 49 cameras, dark images
    dtu = os.path.join(OUT, "scene_dtu", "scan5")
    poses = rig(rng, 49, 0.2)
    write_colmap(dtu, [(1, 1, 8, 6, (10.0, 10.0, 4.0, 3.0))],
                 [(i + 1, poses[i][0], poses[i][1], 1, f"rect_{i + 1:03d}.png") for i in range(49)], (pts[0][:100], pts[1][:100]),
                 text=False)
    for i in range(49):
        a = smooth_image(rng, 6, 8, 3)
        a[:, :3] = rng.integers(0, 40, (6, 3, 3))
        png(os.path.join(dtu, "images", f"rect_{i + 1:03d}.png"), a)
    # Blender
    bl = os.path.join(OUT, "scene_blender")
    os.makedirs(bl, exist_ok=True)
    for split, n in (("train", 94), ("test", 17)):
        frames = []
        for i in range(n):
            th, ph = rng.uniform(0, 2 * np.pi), rng.uniform(0.2, 1.2)
            pos = 4.0 * np.array([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)])
            z = pos / np.linalg.norm(pos)
            x = np.cross([0, 0, 1.0], z)
            x /= np.linalg.norm(x)
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = np.stack([x, np.cross(z, x), z], 1), pos
            stem = ("r_" if split == "train" else "t_") + str(i)           # (distinct names: the records are keyed by name)
            frames.append({"file_path": f"./{split}/{stem}", "transform_matrix": m.tolist()})
            a = smooth_image(rng, 6, 8, 4)
            a[..., 3] = rng.choice([0, 255, 90, 200], (6, 8))
            png(os.path.join(bl, split, stem + ".png"), a)
        with open(os.path.join(bl, f"transforms_{split}.json"), "w") as fp:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, fp)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def prep_source(rng, name, Ws, Hs, C):
    if name.startswith("dtu"):
        a = rng.integers(40, 256, (Hs, Ws, 3), dtype=np.uint8)
        edge = np.array([14, 15, 16, 29, 30, 31, 0, 5, 14, 29], dtype=np.uint8)
        a[:, :10] = edge[None, :, None]                                  # a dark border of constant columns
        a[:, 10:12] = rng.integers(0, 3, (Hs, 2, 3)) * 15                # 0 / 15 / 30 mixed
        a[20:60, 14:18] = 3                                              # a 40-row dark run
        a[30:130, 20:24] = 7                                             # a 100-row one
        a[0:55, 26:28] = 1                                               # from the top edge
        a[5:56, 30] = 2                                                  # 51 rows
        a[5:55, 32] = 2                                                  # 50
        a[5:54, 34] = 2                                                  # 49
        return a
    a = rng.integers(0, 256, (Hs, Ws, C), dtype=np.uint8)
    if C == 4:
        u = rng.random((Hs, Ws))
        a[..., 3] = np.where(u < 0.3, 0, np.where(u < 0.6, 255, a[..., 3]))
    return a[..., 0] if C == 1 else a


def dtu_statements():
    """The text of the DTU block of the reference's train.py, to be executed on CPU tensors"""
    lines = open(os.path.join(REF, "train.py")).read().splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.strip() == "bg_mask = None")
    b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith("####"))
    import textwrap
    return compile(textwrap.dedent("\n".join(lines[a:b])), "train.py[dtu]", "exec")


def main():
    from PIL import Image
    install_shim({})
    rng = np.random.default_rng(14)
    make_folders(rng)
    out = {}
    code = dtu_statements()
    with CudaToCpu():
        from scene import dataset_readers as ref_dr
        from utils import camera_utils as ref_cu
        ref_dr.fetchPly = lambda path: None
        ref_dr.storePly = lambda *a: open(a[0], "wb").close()
        info = lambda img, name="x": types.SimpleNamespace(uid=0, R=np.eye(3), T=np.zeros(3), FovX=0.8, FovY=0.6, image=img,  # noqa: E731
                                                           image_name=name)

        pil_to_torch, forced = ref_cu.PILtoTorch, []
        # (loadCam scales both axes alike; a forced size reaches the cases that leave one axis unchanged)
        ref_cu.PILtoTorch = lambda img, res: pil_to_torch(img, forced[0] if forced else res)

        def load(img, resolution, white, ci=None, size=None):
            args = types.SimpleNamespace(resolution=resolution, white_background=white, data_device="cpu")
            forced[:] = [size] if size else []
            try:
                return ref_cu.loadCam(args, 0, ci if ci is not None else info(img), 1.0)
            finally:
                forced[:] = []

        # (a) preparation
        names = []
        for name, (Ws, Hs), C, (w, h) in PREP:
            src = prep_source(rng, name, Ws, Hs, C)
            names.append(name)
            out[f"prep/{name}/src"] = src
            out[f"prep/{name}/size"] = np.array([w, h])
            for white in (0, 1):
                cam = load(Image.fromarray(src), w, bool(white), size=(w, h))
                assert (cam.image_width, cam.image_height) == (w, h), (name, cam.image_width, cam.image_height)
                if white and cam.gt_alpha_mask is None:
                    assert np.array_equal(out[f"prep/{name}/w0/image"], cam.original_image.numpy())
                    continue                                              # (no alpha: the flag changes nothing; stored once)
                out[f"prep/{name}/w{white}/image"] = cam.original_image.numpy()
                if cam.gt_alpha_mask is not None:
                    out[f"prep/{name}/w{white}/alpha"] = cam.gt_alpha_mask.numpy()
                if name.startswith("dtu") or name in ("rgba_by2", "rgb_by8"):
                    for tag, path in (("30", "/data/scan5"), ("15", "/data/scan110")):
                        env = {"torch": torch, "gt_image": cam.original_image.clone(),
                               "args": types.SimpleNamespace(dataset_name="DTU", source_path=path)}
                        exec(code, env)
                        out[f"prep/{name}/w{white}/bg{tag}"] = env["bg_mask"].numpy().astype(np.uint8)
        out["prep/names"] = np.array(names)
        sizes = []
        for W0, H0 in ((1599, 40), (1600, 40), (1601, 40), (4032, 60), (403, 302), (33, 21), (1700, 50)):
            img = Image.fromarray(np.zeros((H0, W0, 3), np.uint8))
            for r in RESOLUTIONS:
                cam = load(img, r, False)
                sizes.append([W0, H0, r, cam.image_width, cam.image_height])
        out["sizes"] = np.array(sizes)

        # (b) scenes
        def record(tag, si, gt_args=None):
            cams = {c.image_name: c for c in list(si.train_cameras) + list(si.test_cameras)}
            order = sorted(cams)
            out[f"scene/{tag}/names"] = np.array(order)
            out[f"scene/{tag}/train"] = np.array([c.image_name for c in si.train_cameras])
            out[f"scene/{tag}/test"] = np.array([c.image_name for c in si.test_cameras])
            for key, fn in (("R", lambda c: c.R), ("T", lambda c: c.T), ("fov", lambda c: [c.FovX, c.FovY]),
                            ("wh", lambda c: [c.width, c.height]), ("uid", lambda c: c.uid)):
                out[f"scene/{tag}/{key}"] = np.array([fn(cams[n]) for n in order])
            out[f"scene/{tag}/radius"] = np.array(si.nerf_normalization["radius"])
            out[f"scene/{tag}/translate"] = np.array(si.nerf_normalization["translate"])
            out[f"scene/{tag}/ply_path"] = np.array(si.ply_path)
            camlist = list(si.test_cameras) + list(si.train_cameras)
            out[f"scene/{tag}/cameras_json"] = np.array(json.dumps([ref_cu.camera_to_JSON(i, c) for i, c in enumerate(camlist)]))
            if gt_args:
                for c in camlist:
                    cam = load(None, gt_args[0], gt_args[1], c)
                    out[f"scene/{tag}/gt/{c.image_name}/image"] = cam.original_image.numpy()
                    if cam.gt_alpha_mask is not None:
                        out[f"scene/{tag}/gt/{c.image_name}/alpha"] = cam.gt_alpha_mask.numpy()

        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            for folder in ("LLFF", "DTU"):
                os.makedirs(os.path.join("keypoints_to_3d", folder))
            for f in ("LLFF/scene_llff", "LLFF/scene_llff_txt", "DTU/scan5"):
                open(f"keypoints_to_3d/{f}_keypoints_to_3d.ply", "wb").close()
            rel = lambda *p: os.path.join(OUT, *p)  # noqa: E731
            try:
                record("llff_n3", ref_dr.readColmapSceneInfo(rel("scene_llff"), "images", True, 3, "LLFF"), (2, False))
                record("llff_n0", ref_dr.readColmapSceneInfo(rel("scene_llff"), "images", True, 0, "LLFF"))
                record("llff_txt_n3", ref_dr.readColmapSceneInfo(rel("scene_llff_txt"), "images", True, 3, "LLFF"))
                record("dtu_n3", ref_dr.readColmapSceneInfo(rel("scene_dtu", "scan5"), "images", True, 3, "DTU"))
                np.random.seed(0)
                record("blender_n3", ref_dr.readNerfSyntheticInfo(rel("scene_blender"), True, True, 3, "Blender"), (4, True))
                record("blender_all", ref_dr.readNerfSyntheticInfo(rel("scene_blender"), True, False, 3, "Blender"))
            finally:
                os.chdir(cwd)
                for stray in (rel("scene_llff", "sparse/0/points3D.ply"), rel("scene_llff_txt", "sparse/0/points3D.ply"),
                              rel("scene_dtu", "scan5", "sparse/0/points3D.ply"), rel("scene_blender", "points3d.ply")):
                    if os.path.exists(stray):
                        os.remove(stray)
    path = os.path.join(OUT, "scene_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
