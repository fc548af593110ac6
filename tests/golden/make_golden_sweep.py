#!/usr/bin/env python
"""Writes golden G16, tests/golden/sweep.npz: the plane-sweep matcher's yardstick (tests/sweep_ref.py, float64) on the synthetic
scene of sweep_ref.make_scene() -- three 96x72 pinhole cameras, a slanted textured plane, a nearer plane in front of part of it
and a periodic stripe region -- at stride 2, D = 32.  CPU only; run from the repository root:

    python tests/golden/make_golden_sweep.py

The maker asserts, ON THE FLOAT64 RESTATEMENT ALONE, the conditions the tests lean on, and fails when the scene does not meet
them (then the scene is changed, not the caps):
  (a) < 2 % of the nodes are near-ties: a decision of theirs -- the top two scores, a threshold, a tap on the frame's edge, the
      rounding of the left/right lookup -- lies within sweep_ref.NEAR_TIE / EDGE_TIE of flipping.  Tests may leave these out.
  (b) < 5 % of the returned matches lie more than 1 px from the true correspondence
  (c) matches come back for at least half of the textured, unoccluded nodes
  (d) none comes back inside the striped region
  (e) err32 = the largest |float32 restatement - float64 restatement| over all scores valid in both; 4 err32 < NEAR_TIE, so that
      a kernel within 4 err32 of the yardstick cannot reorder scores that are not near-ties
  (f) < 5 % of the returned matches have an inverse depth a hypothesis step or more from the truth (the end-to-end test's bound)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sweep_ref as sr  # noqa: E402

PARAMS = sr.Params(stride=2, hypotheses=32)
PAIRS = ((0, 1), (0, 2), (1, 2))


def figures(sc, images, params=PARAMS, pairs=PAIRS, with32=True):
    """-> (arrays to store, totals) of the restatement on a scene"""
    out, tot, err32 = {}, dict(nodes=0, near_ties=0, returned=0, off_1px=0, off_step=0, eligible=0, eligible_returned=0, striped=0,
                               striped_returned=0), 0.0
    for a, b in pairs:
        args = (images[a], images[b], sc.K, sr.w2c(sc, a), sr.w2c(sc, b), sc.near, sc.far, params)
        r64 = sr.match_pair(*args, T=np.float64)
        r32 = sr.match_pair(*args, T=np.float32) if with32 else None
        for d, (x, y) in enumerate(((a, b), (b, a))):
            tag = f"dir/{x}_{y}/"
            sel, dr, tr = r64.sel[d], r64.dirs[d], sr.truth(sc, x, y, params.stride)
            if with32:
                both = r64.vols[d].valid & r32.vols[d].valid
                err32 = max(err32, float(np.abs(r64.vols[d].scores - r32.vols[d].scores.astype(np.float64))[both].max()))
            step = float(sr.plan(sc.K, sr.w2c(sc, x), sr.w2c(sc, y), sc.near, sc.far, params.hypotheses).step)
            off = np.linalg.norm(dr.q - tr.q, axis=1)
            tot["nodes"] += len(off)
            tot["near_ties"] += int(dr.fragile.sum())
            tot["returned"] += int(dr.keep.sum())
            tot["off_1px"] += int((off[dr.keep] > 1.0).sum())
            tot["off_step"] += int((np.abs(sel.invd - 1.0 / tr.z)[dr.keep] >= step).sum())
            tot["eligible"] += int(tr.eligible.sum())
            tot["eligible_returned"] += int((tr.eligible & dr.keep).sum())
            tot["striped"] += int(tr.striped.sum())
            tot["striped_returned"] += int((tr.striped & dr.keep).sum())
            out.update({tag + "has": sel.has, tag + "k": sel.k.astype(np.int32), tag + "best": sel.best, tag + "lcr": sel.lcr,
                        tag + "refined": sel.refined, tag + "invd": sel.invd, tag + "keep": dr.keep, tag + "q": dr.q,
                        tag + "near_tie": dr.fragile, tag + "any_valid": r64.vols[d].valid.any(axis=0), tag + "true_q": tr.q,
                        tag + "true_z": tr.z, tag + "eligible": tr.eligible, tag + "striped": tr.striped, tag + "step": np.float64(step)})
    tot["err32"] = err32
    return out, tot


def check(tot):
    print(tot)
    assert tot["near_ties"] < 0.02 * tot["nodes"], "(a)"
    assert tot["off_1px"] < 0.05 * tot["returned"], "(b)"
    assert tot["eligible_returned"] >= 0.5 * tot["eligible"] and tot["eligible"] > 0, "(c)"
    assert tot["striped"] > 100 and tot["striped_returned"] == 0, "(d)"
    assert 0 < 4 * tot["err32"] < sr.NEAR_TIE, "(e)"
    assert tot["off_step"] < 0.05 * tot["returned"], "(f)"


def main():
    sc = sr.make_scene()
    images = np.stack([sr.render(sc, v) for v in range(len(sc.c2ws))])
    out, tot = figures(sc, images)
    check(tot)
    out.update({"images": images, "K": sc.K, "c2ws": sc.c2ws, "near": np.float64(sc.near), "far": np.float64(sc.far),
                "stride": np.int32(PARAMS.stride), "hypotheses": np.int32(PARAMS.hypotheses), "pairs": np.array(PAIRS, np.int32),
                "err32": np.float64(tot["err32"]), "totals": np.array([f"{k}={v}" for k, v in tot.items()])})
    path = os.path.join(HERE, "sweep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
