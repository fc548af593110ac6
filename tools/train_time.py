#!/usr/bin/env python
"""usage (GPU box): python tools/train_time.py [SCENE_FOLDER | synth] [P W H] [--dataset_name LLFF] [-r RES] [--rounds 8] [--block 40]

`train --step schedule` against `train --step graph`: schedule.IterationSchedule and graph_trainer.GraphTrainer, each on its
own copy of the same model, run INTERLEAVED in blocks of `--block` iterations inside one process (the pattern of
tools/ab_interleaved.py: two separate runs differ by +-15 % on a shared host), single-view iterations (before
--shift_cam_start) and pair iterations (after it) separately.  Per mode and phase: median and best block in iterations/s,
and the spread of the blocks -- a gap below the spread is "no difference".  Densification, reports and the SH raise are
pushed out of the measured span (they are the same statements in both modes); the opacity decay is on, as in a default run.

    SCENE_FOLDER   a dataset folder read by Scene.from_dataset (default tests/golden/scene_llff, --init_points sparse)
    synth P W H    a synthetic scene as bench_ref_schedule.py builds it (default 500000 504 378), random ground truth
The last line is one JSON object with every figure."""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIR_FROM = 1_000_000          # shift_cam_start: iterations below it are single-view, above it pairs
FAR = 10 ** 9


def _training_args():
    from binocular3dgs_amd import train
    return train.parser().parse_args([])


def _folder(path, a, dev):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    random.seed(0)
    model = GaussianModel(1)
    scene = Scene.from_dataset(path, model, eval=True, n_views=3, dataset_name=a.dataset_name, resolution=a.resolution,
                               init_points="sparse", device=dev)
    model.training_setup(_training_args())
    return model, scene


def _synth(P, W, H, dev):
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.scene import Scene
    model = synth.synth_model(P, seed=0, device=dev, width=W, height=H, fovx_deg=60.0)
    cams = synth.synth_cameras(W, H, fovx_deg=60.0, yaws=synth.YAWS_6, device=dev)[:3]
    g = torch.Generator(device="cpu").manual_seed(11)
    for c in cams:
        c.original_image, c.gt_alpha_mask = torch.rand((3, H, W), generator=g).to(dev), None
    model.spatial_lr_scale = 1.0
    model.training_setup(_training_args())
    return model, Scene(cams, model, cameras_extent=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default=os.path.join(ROOT, "tests", "golden", "scene_llff"))
    ap.add_argument("size", nargs="*", type=int, default=[500_000, 504, 378])
    ap.add_argument("--dataset_name", default="LLFF")
    ap.add_argument("--resolution", "-r", type=int, default=-1)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=40)
    a = ap.parse_args()
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    from binocular3dgs_amd.render import PipelineParams
    from binocular3dgs_amd.schedule import IterationSchedule
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bg = torch.zeros(3, device=dev)
    kw = dict(iterations=FAR, shift_cam_start=PAIR_FROM, binocular=True, opacity_decay_factor=0.995, lambda_dssim=0.2,
              densify_from_iter=0, densify_until_iter=FAR, densification_interval=FAR, sh_interval=FAR)
    trainers = {}
    for mode, cls in (("schedule", IterationSchedule), ("graph", GraphTrainer)):
        model, scene = _synth(*a.size, dev) if a.scene == "synth" else _folder(a.scene, a, dev)
        trainers[mode] = cls(model, scene, PipelineParams(), bg, **kw)
    views = trainers["graph"].views
    what = {"scene": a.scene, "points": int(trainers["graph"].model.get_xyz.shape[0]),
            "size": [views[0].image_width, views[0].image_height], "rounds": a.rounds, "block": a.block}
    rng = random.Random(5)
    clock = {("schedule", "single"): 1000, ("schedule", "pair"): PAIR_FROM + 1000}
    clock.update({("graph", p): v for (_, p), v in list(clock.items())})

    def run(mode, phase, n):
        tr = trainers[mode]
        for _ in range(n):
            clock[mode, phase] += 1
            tr.run_iteration(clock[mode, phase], rng.randrange(len(views)), rng.random() * 0.4 * rng.choice([-1.0, 1.0]))

    res = {}
    for phase in ("single", "pair"):
        blocks = {m: [] for m in trainers}
        for _ in range(a.rounds):
            for mode in trainers:
                run(mode, phase, 8)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(mode, phase, a.block)
                torch.cuda.synchronize(dev)
                blocks[mode].append(a.block / (time.perf_counter() - t0))
        for mode, v in blocks.items():
            res[f"{phase}/{mode}"] = {"median": round(statistics.median(v), 1), "best": round(max(v), 1),
                                      "worst": round(min(v), 1)}
            print(f"{phase:6s} {mode:8s} median {statistics.median(v):8.1f} it/s   best {max(v):8.1f}   blocks {min(v):.1f}..{max(v):.1f}")
        s, g = res[f"{phase}/schedule"], res[f"{phase}/graph"]
        spread = max(s["best"] - s["worst"], g["best"] - g["worst"])
        gap = g["median"] - s["median"]
        res[f"{phase}/verdict"] = "no difference" if abs(gap) <= spread else ("graph faster" if gap > 0 else "graph SLOWER")
        print(f"{phase:6s} graph / schedule = {g['median'] / s['median']:.2f}  (gap {gap:+.1f} it/s, block spread {spread:.1f}): "
              f"{res[phase + '/verdict']}")
    gt = trainers["graph"]
    gt.settle()
    what.update(res, captures=gt.captures, grown=gt.grown)
    print(json.dumps(what))


if __name__ == "__main__":
    main()
