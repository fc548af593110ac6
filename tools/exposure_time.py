"""Times exposure compensation (binocular3dgs_amd/exposure.py): apply + backward for one 800x600 plane and for the trainers' pair
(two planes that share a matrix: one apply launch, one backward launch) against the float32 torch restatement (upstream's
statement: matmul + permute, autograd backward), in milliseconds and device launches; then the graph-replayed training step
(graph_trainer.GraphTrainer on the synthetic scene of the trainer tests) with the term on and off.  The alternatives alternate
in blocks in one process, as tools/ab_interleaved.py does; medians over the blocks.

    python tools/exposure_time.py [--blocks 9] [--calls 50] [--iters 200]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def restated(image, A):
    """upstream: torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None], with
    this project's row convention (out_c = sum_k A[c][k] x_k + A[c][3])"""
    return torch.matmul(image.permute(1, 2, 0), A[:, :3].t()).permute(2, 0, 1) + A[:, 3, None, None]


def launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    on_device = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(e.count for e in on_device), sum(e.count for e in on_device if "exposure_" in e.key)


def interleaved(fns, blocks, calls):
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls * 1e3)
    return {name: statistics.median(v) for name, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    args = ap.parse_args(argv)
    from binocular3dgs_amd.exposure import apply_exposure_batch
    dev, W, H = "cuda:0", args.width, args.height
    g = torch.Generator(device=dev).manual_seed(0)
    for n in (1, 2):
        images = [torch.rand((3, H, W), device=dev, generator=g).requires_grad_(True) for _ in range(n)]
        grads = [torch.randn((3, H, W), device=dev, generator=g) for _ in range(n)]
        A = (torch.eye(3, 4, device=dev) + 0.1 * torch.randn((3, 4), device=dev, generator=g)).requires_grad_(True)

        def hip():
            torch.autograd.backward(apply_exposure_batch(images, [A] * n, slot="time"), grads)

        def torch32():
            torch.autograd.backward([restated(x, A) for x in images], grads)

        ms = interleaved({"hip": hip, "restatement": torch32}, args.blocks, args.calls)
        lh, lr = launches(hip), launches(torch32)
        print(f"{n} plane(s) {W}x{H}, apply + backward: hip {ms['hip']:.4f} ms ({lh[1]} library launches, {lh[0]} device launches with "
              f"autograd's), restatement {ms['restatement']:.4f} ms ({lr[0]} device launches)")

    import ref_schedule as rs
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    from test_gpu_exposure import Lead
    scene = rs.make_scene()
    runs = {"term on": Lead(GraphTrainer, scene, check_every=0x7fffffff), "term off": Lead(GraphTrainer, scene, exposure=False, check_every=0x7fffffff)}
    it = {name: 0 for name in runs}
    for lead in runs.values():
        lead.run(8)                                                   # both shapes captured: single view, then the pair
    it = {name: 8 for name in runs}

    def stepper(name):
        def step():
            lead = runs[name]
            it[name] += 1
            k = 5 + it[name] % 400                                    # (pair iterations; the schedule's numbers stay small)
            lead.tr.run_iteration(k, int(lead.views[k]), float(lead.shifts[k]))
        return step
    ms = interleaved({name: stepper(name) for name in runs}, args.blocks, args.iters)
    for lead in runs.values():
        lead.tr.settle()
    print("graph step, " + ", ".join(f"{name}: {1e3 / v:.0f} iterations / s ({v:.4f} ms)" for name, v in ms.items())
          + f"; captures {[lead.tr.captures for lead in runs.values()]}")


if __name__ == "__main__":
    main()
