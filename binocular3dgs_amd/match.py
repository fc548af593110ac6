"""python -m binocular3dgs_amd.match --data_path SRC --output FILE.npz [--dataset_name LLFF --n_views 3 --resolution 4
--sweep_stride 2 --sweep_hypotheses 128 --near N --far F --min_score 0.8]

Writes only the match file of the plane-sweep matcher (sweep_matcher.py; not the reference's network): the
kp_<ref>_<src>_source / _target arrays that `keypoints_to_3d --matches FILE.npz` and the reference's own triangulation
script read."""
from __future__ import annotations

import argparse
import sys

from .keypoints_to_3d import add_sweep_arguments, sweep_params
from .matcher_cloud import DTU_SPARSE_INDICES


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Plane-sweep stereo matches of a dataset folder")
    p.add_argument("--data_path", type=str, required=True)
    p.add_argument("--output", type=str, required=True, help="the .npz to write")
    add_sweep_arguments(p)
    p.add_argument("--n_views", type=int, default=3)
    p.add_argument("--resolution", type=int, default=4)
    p.add_argument("--dtu_sparse_indices", type=int, nargs="+", default=list(DTU_SPARSE_INDICES))
    p.add_argument("--dataset_name", type=str, default="LLFF", choices=["LLFF", "DTU"])
    return p


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    from .sweep_matcher import match_views, write_matches
    matches = match_views(args.data_path, dataset_name=args.dataset_name, n_views=args.n_views, resolution=args.resolution,
                          dtu_sparse_indices=args.dtu_sparse_indices, params=sweep_params(args))
    write_matches(args.output, matches)
    print(f"matches: {args.output} ({sum(len(v) for k, v in matches.items() if k.endswith('_source'))} in {len(matches) // 2} ordered pairs)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
