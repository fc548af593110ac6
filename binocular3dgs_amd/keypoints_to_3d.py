"""python -m binocular3dgs_amd.keypoints_to_3d --data_path SRC --matches FILE.npz [--dataset_name LLFF --n_views 3
--resolution 4 --output_path keypoints_to_3d/LLFF --seed 0]
python -m binocular3dgs_amd.keypoints_to_3d --data_path SRC --matcher sweep [--sweep_stride 2 --sweep_hypotheses 128 --near N
--far F --min_score 0.8 --save_matches FILE.npz] [...]

Writes <output_path>/<scene>_keypoints_to_3d.ply, the file `--init_points matcher` reads, from the keypoint matches of a
dense matcher (format: matcher_cloud's docstring).  The flags are those of the reference's triangulate.py where they still
mean something; the matcher's own flags are gone with the matcher.  `--matcher file` (the default) reads the matches of
`--matches`; `--matcher sweep` computes them with the plane-sweep matcher of sweep_matcher.py, which needs no weights and is
not the reference's network."""
from __future__ import annotations

import argparse
import os
import sys

from .matcher_cloud import DTU_SPARSE_INDICES


def add_sweep_arguments(p: argparse.ArgumentParser) -> None:
    p.add_argument("--sweep_stride", type=int, default=2, help="a node every this many pixels")
    p.add_argument("--sweep_hypotheses", type=int, default=128, help="inverse-depth planes between --near and --far")
    p.add_argument("--near", type=float, default=None, help="depth range of the sweep (default: from the COLMAP points of sparse/0)")
    p.add_argument("--far", type=float, default=None)
    p.add_argument("--min_score", type=float, default=0.8, help="smallest ZNCC of a match")


def sweep_params(args):
    from .sweep_matcher import SweepParams
    return SweepParams(stride=args.sweep_stride, hypotheses=args.sweep_hypotheses, min_score=args.min_score, near=args.near, far=args.far)


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if a.matcher == "file" and a.matches is None:
            self.error("the following arguments are required: --matches (with --matcher file)")
        if a.matcher == "sweep" and a.matches is not None:
            self.error("--matches belongs to --matcher file; --matcher sweep computes the matches (--save_matches writes them)")
        return a


def parser() -> argparse.ArgumentParser:
    p = _Parser(description="Triangulate script parameters")
    p.add_argument("--data_path", type=str, required=True)
    p.add_argument("--matches", type=str, default=None, help="the .npz of kp_<ref>_<src>_source / _target arrays (--matcher file)")
    p.add_argument("--matcher", type=str, default="file", choices=["file", "sweep"],
                   help="file: the matches of --matches; sweep: the plane-sweep matcher (no weights; not the reference's network)")
    add_sweep_arguments(p)
    p.add_argument("--save_matches", type=str, default=None, help="--matcher sweep: also write the matches to this .npz")
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
    how = {} if args.matcher == "file" else {"matcher": "sweep", "sweep": sweep_params(args), "save_matches": args.save_matches}
    xyz, rgb = build_cloud(args.data_path, args.matches, dataset_name=args.dataset_name, n_views=args.n_views,
                           resolution=args.resolution, dtu_sparse_indices=args.dtu_sparse_indices, iterations=args.iterations, **how)
    path = output_file(args)
    write_cloud_ply(path, xyz, rgb)
    print(f"export: {path} ({len(xyz)} points)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
