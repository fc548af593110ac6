"""Store a trained model cheaply: sensitivity-weighted vector quantisation of its colour rows and of its shape rows.

The method is the one of Niedermayr et al., "Compressed 3D Gaussian Splatting" (2024), and of LightGaussian's VecTree step
(Fan et al., 2023): cluster the colour rows and the shape rows with k-means, every row weighted by what the Gaussian is worth
to the renders (importance.Contributions.weight), and keep two small codebooks and one 16-bit index per Gaussian per group.
The clustering is Lloyd's algorithm on the device (csrc/kmeans.hip: the assignment is a GEMM with an argmin epilogue on the
exact-f32 MFMA, the update an ordered fp64 sum); there is no host statement of it in the package.

    colour row  _features_dc (+) _features_rest, flattened:  D = 12 at SH degree 1, 48 at degree 3
    shape row   _scaling (+) the rotation, normalised and sign-canonical (canonical_rotation):  D = 7
    _xyz stays float32, _opacity (the logit) becomes float16, indices are uint16, codebooks float32.

Caveat: q and -q are the same rotation, and the renderer normalises; the stored rotation is the unit quaternion with w >= 0
(then the first non-zero component positive), not the raw parameter.  A decompressed model renders what the model with
canonical_rotation(_rotation) in place of _rotation renders -- bit for bit when every row has its own code -- which differs from
the original's render by the rounding of one more normalisation.

File: one .npz (numpy.savez_compressed) with the arrays of CompressedModel, `sh_degree`, `active_sh_degree` and
`format_version`; save_compressed / load_compressed are pure numpy and work without a device.

python -m binocular3dgs_amd.compress -m MODEL_PATH [-s SOURCE] [--iteration N] [--pruned] [--colour_codes K] [--shape_codes K]
      [--iters I] [--views train|test|all | --uniform] [--evaluate] [--decompress]

Loads the model as prune.py does (--pruned: from iteration_<n>_pruned), takes the weights from importance.contributions over the
chosen cameras (--uniform: all ones, no cameras are read unless --evaluate), writes
<MODEL_PATH>/point_cloud/iteration_<n>_compressed/model.npz and, with --decompress, point_cloud.ply next to it (what every other
command line reads).  Prints one JSON line: P, bytes before and after and their ratio, the distortion series of both groups;
with --evaluate the evaluate_views means (mode "report") of the test cameras before and after.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

FORMAT_VERSION = 1
MAX_CODES = 65536
_PAYLOAD = ("xyz", "opacity", "colour_codebook", "colour_index", "shape_codebook", "shape_index")


@dataclass
class CompressedModel:
    xyz: np.ndarray                 # [P,3] float32
    opacity: np.ndarray             # [P,1] float16, the logit
    colour_codebook: np.ndarray     # [Kc, 3 (sh_degree + 1)^2] float32
    colour_index: np.ndarray        # [P] uint16
    shape_codebook: np.ndarray      # [Ks,7] float32: log-scaling (3), canonical unit quaternion (4)
    shape_index: np.ndarray         # [P] uint16
    colour_distortion: np.ndarray   # [iters + 1] float64: weighted squared error of every assignment
    shape_distortion: np.ndarray    # [iters + 1] float64
    sh_degree: int
    active_sh_degree: int


def kmeans(x, k: int, weights=None, iters: int = 10, init=None, seed: int = 0):
    """Weighted Lloyd iterations of the rows x [N,D] (1 <= D <= 64) on the device -> (codebook float32 [K,D], codes int32 [N],
    counts int32 [K], distortion float64 [iters + 1]); distortion[i] belongs to assignment i, the codes to the returned codebook.
    init: [K,D] initial codes; None: the rows at the sorted first k entries of torch.randperm(N) of a CPU generator seeded with
    `seed` -- all rows in order when k >= N (the codebook then has N entries, every row its own code)."""
    import torch
    from . import _C
    if x.dim() != 2:
        raise ValueError("kmeans: x is [N,D]")
    N = x.shape[0]
    if init is None:
        if k < 1:
            raise ValueError("kmeans: k >= 1")
        if k >= N:
            init = x
        else:
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
            init = x[torch.sort(perm[:k]).values.to(x.device)]
    w = None if weights is None else weights.detach().reshape(-1).to(torch.float32)
    return _C.kmeans(x.detach(), w, init.detach(), int(iters))


def assign(x, codebook):
    """codes int32 [N]: for every row of x [N,D] the nearest row of codebook [K,D] (the lower k of equal scores)."""
    from . import _C
    return _C.kmeans_assign(x.detach(), codebook.detach())


def canonical_rotation(rotation):
    """[P,4] -> the unit quaternion of the same rotation with w >= 0, then the first non-zero component positive."""
    import torch
    q = torch.nn.functional.normalize(rotation.detach().float())
    nz = q != 0
    first = torch.argmax(nz.to(torch.int8), dim=1, keepdim=True)         # the first non-zero component (0 when there is none)
    lead = torch.gather(q, 1, first)
    return torch.where(lead < 0, -q, q)


def group_rows(model):
    """-> (colour [P, 3 (sh_degree + 1)^2], shape [P,7]) float32: the rows the two codebooks are made of."""
    import torch
    P = model._xyz.shape[0]
    colour = torch.cat([model._features_dc.detach().reshape(P, -1), model._features_rest.detach().reshape(P, -1)], dim=1).float()
    shape = torch.cat([model._scaling.detach().float(), canonical_rotation(model._rotation)], dim=1)
    return colour.contiguous(), shape.contiguous()


def compress(model, weights=None, colour_codes: int = 4096, shape_codes: int = 4096, iters: int = 10, seed: int = 0) -> CompressedModel:
    """weights: importance.Contributions.weight or any [P] tensor (cast to float32), None = uniform."""
    for k in (colour_codes, shape_codes):
        if not 1 <= k <= MAX_CODES:
            raise ValueError(f"1 <= codes <= {MAX_CODES}: the indices are 16-bit words")
    P = model._xyz.shape[0]
    if P == 0:
        raise ValueError("compress: the model is empty")
    if weights is not None and weights.numel() != P:
        raise ValueError("one weight per Gaussian")
    colour, shape = group_rows(model)
    cc, ci, _, cd = kmeans(colour, colour_codes, weights, iters, seed=seed)
    sc, si, _, sd = kmeans(shape, shape_codes, weights, iters, seed=seed)

    def host(t, dtype):
        return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))
    return CompressedModel(xyz=host(model._xyz, np.float32), opacity=host(model._opacity.reshape(P, 1), np.float16),
                           colour_codebook=host(cc, np.float32), colour_index=host(ci, np.uint16),
                           shape_codebook=host(sc, np.float32), shape_index=host(si, np.uint16),
                           colour_distortion=host(cd, np.float64), shape_distortion=host(sd, np.float64),
                           sh_degree=int(model.max_sh_degree), active_sh_degree=int(model.active_sh_degree))


def decompress(cm: CompressedModel, device="cuda", requires_grad: bool = False):
    """A GaussianModel of the stored rows (GaussianModel.from_tensors)."""
    import torch
    from .gaussian_model import GaussianModel
    P = cm.xyz.shape[0]
    colour = torch.from_numpy(cm.colour_codebook)[torch.from_numpy(cm.colour_index.astype(np.int64))]
    shape = torch.from_numpy(cm.shape_codebook)[torch.from_numpy(cm.shape_index.astype(np.int64))]
    return GaussianModel.from_tensors(torch.from_numpy(cm.xyz), colour[:, :3].reshape(P, 1, 3), colour[:, 3:].reshape(P, -1, 3),
                                      shape[:, :3], shape[:, 3:], torch.from_numpy(cm.opacity.astype(np.float32)),
                                      sh_degree=cm.sh_degree, active_sh_degree=cm.active_sh_degree, device=device,
                                      requires_grad=requires_grad)


def _checked(cm: CompressedModel) -> CompressedModel:
    P = cm.xyz.shape[0]
    want = dict(xyz=(np.float32, (P, 3)), opacity=(np.float16, (P, 1)), colour_index=(np.uint16, (P,)), shape_index=(np.uint16, (P,)))
    for name, (dtype, shape) in want.items():
        a = getattr(cm, name)
        if a.dtype != dtype or a.shape != shape:
            raise ValueError(f"CompressedModel.{name} must be {np.dtype(dtype).name} {shape}, not {a.dtype} {a.shape}")
    dc = 3 * (cm.sh_degree + 1) ** 2
    for name, d, idx in (("colour_codebook", dc, cm.colour_index), ("shape_codebook", 7, cm.shape_index)):
        a = getattr(cm, name)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != d or not 1 <= a.shape[0] <= MAX_CODES:
            raise ValueError(f"CompressedModel.{name} must be float32 [K,{d}] with 1 <= K <= {MAX_CODES}")
        if P and int(idx.max()) >= a.shape[0]:
            raise ValueError(f"an index points past CompressedModel.{name}")
    return cm


def save_compressed(path: str, cm: CompressedModel) -> None:
    _checked(cm)
    arrays = {f.name: np.asarray(getattr(cm, f.name)) for f in fields(cm)}
    with open(path, "wb") as fp:                      # (a file object: numpy appends no ".npz" to the name)
        np.savez_compressed(fp, format_version=np.int32(FORMAT_VERSION), **arrays)


def load_compressed(path: str) -> CompressedModel:
    with np.load(path) as z:
        if "format_version" not in z or int(z["format_version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: not a compressed model of format version {FORMAT_VERSION}")
        cm = CompressedModel(**{f.name: (int(z[f.name]) if f.type == "int" else np.array(z[f.name])) for f in fields(CompressedModel)})
    return _checked(cm)


def compressed_bytes(cm: CompressedModel) -> int:
    """Bytes of the arrays a decompression needs (before the file's own deflate)."""
    return int(sum(getattr(cm, name).nbytes for name in _PAYLOAD))


def model_bytes(model) -> int:
    """Bytes of a full float32 model: 92 per Gaussian at SH degree 1, 236 at degree 3."""
    return int(4 * sum(p.numel() for p in (model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation,
                                            model._opacity)))


def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, pruned: bool = False, colour_codes: int = 4096,
        shape_codes: int = 4096, iters: int = 10, views: str = "train", uniform: bool = False, evaluate: bool = False,
        decompress_ply: bool = False, seed: int = 0) -> dict:
    import torch
    from . import importance
    from .evaluate import evaluate_views
    from .gaussian_model import GaussianModel
    from .scene import Scene
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    folder = os.path.join(model_path, "point_cloud", "iteration_" + str(it))
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(folder + ("_pruned" if pruned else ""), "point_cloud.ply"))
    white = bool(cfg.get("white_background", False))
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    weights, test = None, []
    if not uniform or evaluate:
        source_path = source_path or cfg.get("source_path")
        if not source_path:
            raise ValueError("no source path: pass -s or keep cfg_args next to the model")
        scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                                   dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                                   resolution=cfg.get("resolution", -1), white_background=white,
                                   init_points=cfg.get("init_points", "matcher"), shuffle=False)
        train, test = list(scene.getTrainCameras()), list(scene.getTestCameras())
        if not uniform:
            cams = {"train": train, "test": test, "all": train + test}[views]
            if not cams:
                raise ValueError(f"{source_path}: no {views} cameras")
            weights = importance.contributions(model, cams, bg).weight
    cm = compress(model, weights, colour_codes, shape_codes, iters, seed)
    out_dir = folder + "_compressed"
    os.makedirs(out_dir, exist_ok=True)
    npz = os.path.join(out_dir, "model.npz")
    save_compressed(npz, cm)
    before, after = model_bytes(model), compressed_bytes(cm)
    res = {"P": int(cm.xyz.shape[0]), "bytes_before": before, "bytes_after": after, "ratio": before / after,
           "file_bytes": os.path.getsize(npz), "colour_codes": int(cm.colour_codebook.shape[0]),
           "shape_codes": int(cm.shape_codebook.shape[0]), "colour_distortion": [float(v) for v in cm.colour_distortion],
           "shape_distortion": [float(v) for v in cm.shape_distortion], "iteration": it, "weights": "uniform" if uniform else views,
           "npz": npz}
    small = None
    if decompress_ply or evaluate:
        small = decompress(load_compressed(npz))
    if decompress_ply:
        res["ply"] = os.path.join(out_dir, "point_cloud.ply")
        small.save_ply(res["ply"])
    if evaluate:
        if not test:
            raise ValueError(f"{source_path}: --evaluate needs test cameras")
        for tag, m in (("before", model), ("after", small)):
            e = evaluate_views(m, test, bg, mode="report")
            res[tag] = {k: e[k] for k in ("PSNR", "SSIM", "L1")}
    print(json.dumps(res))
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.compress", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--pruned", action="store_true", help="compress iteration_<n>_pruned, what prune.py wrote")
    p.add_argument("--colour_codes", type=int, default=4096)
    p.add_argument("--shape_codes", type=int, default=4096)
    p.add_argument("--iters", type=int, default=10)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--views", choices=("train", "test", "all"), default=None, help="cameras of the contribution weights (train)")
    g.add_argument("--uniform", action="store_true", help="weight every Gaussian alike")
    p.add_argument("--evaluate", action="store_true")
    p.add_argument("--decompress", action="store_true", help="also write point_cloud.ply next to model.npz")
    a = p.parse_args(argv)
    run(a.model_path, a.source_path, a.iteration, a.pruned, a.colour_codes, a.shape_codes, a.iters, a.views or "train", a.uniform,
        a.evaluate, a.decompress)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
