"""python -m binocular3dgs_amd.keypoints_to_3d --data_path SRC --matches FILE.npz [--dataset_name LLFF --n_views 3
--resolution 4 --output_path keypoints_to_3d/LLFF --seed 0]

Writes <output_path>/<scene>_keypoints_to_3d.ply, the file `--init_points matcher` reads, from the keypoint matches of a
dense matcher (format: matcher_cloud's docstring).  The flags are those of the reference's triangulate.py where they still
mean something; the matcher's own flags are gone with the matcher."""
from __future__ import annotations

import argparse
import os
import sys

from .matcher_cloud import DTU_SPARSE_INDICES


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Triangulate script parameters")
    p.add_argument("--data_path", type=str, required=True)
    p.add_argument("--matches", type=str, required=True, help="the .npz of kp_<ref>_<src>_source / _target arrays")
    p.add_argument("--n_views", type=int, default=3)
    p.add_argument("--resolution", type=int, default=4)
    p.add_argument("--dtu_sparse_indices", type=int, nargs="+", default=list(DTU_SPARSE_INDICES))
    p.add_argument("--output_path", type=str, default="keypoints_to_3d")
    p.add_argument("--dataset_name", type=str, default="LLFF", choices=["LLFF", "DTU"])
    p.add_argument("--iterations", type=int, default=1000, help="growth rounds (LLFF)")
    p.add_argument("--seed", type=int, default=0)
    return p


def output_file(args) -> str:
    scene = os.path.basename(os.path.normpath(args.data_path))
    return os.path.join(args.output_path, f"{scene}_keypoints_to_3d.ply")


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    import torch
    from .matcher_cloud import build_cloud, write_cloud_ply
    torch.manual_seed(args.seed)
    xyz, rgb = build_cloud(args.data_path, args.matches, dataset_name=args.dataset_name, n_views=args.n_views,
                           resolution=args.resolution, dtu_sparse_indices=args.dtu_sparse_indices, iterations=args.iterations)
    path = output_file(args)
    write_cloud_ply(path, xyz, rgb)
    print(f"export: {path} ({len(xyz)} points)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
