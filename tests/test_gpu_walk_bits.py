"""The four second walks of a forward's tile lists (csrc/contrib.hip, pixelmaps.hip, segment.hip over csrc/tile_walk.h) against
bits recorded before the walk became one function.

Every result is a deterministic function of the forward's state: the contribution statistics and the votes are integer sums
and maxima (order-free), the pixel maps and the label render are per-pixel float32 sums in list order.  So a refactor of the
walk reproduces the bits, and tests/golden/walk_bits.json holds their SHA-256 per (scene, kernel setting), written once by
tests/golden/make_walk_bits.py on the commit before tile_walk.h and never regenerated from the code under test.  Each scene
also records the hash of the forward's n_contrib: when that differs, the input state differs and the walk is not what changed.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import helpers
import segment_ref
from test_gpu_contrib import KEYS, Device
from test_gpu_pixelmaps import PLANES, pixel_maps
from test_gpu_segment import label_render, label_votes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_bits.json")
SCENES = ("stack257", "stack513", "cull_75x33", "ladder_b", "two_segments")
VOTE_LABELS = (2, 16)
RENDER_LABELS = (2, 4, 8, 16)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def walk_hashes(scene):
    """One forward of `scene`, every kernel setting once -> {setting: {array: sha256}} (and "n_contrib": sha256)."""
    if scene == "two_segments":
        d, frac = helpers.two_segment_scene(), 0.5
    elif scene == "cull_75x33":
        d, frac = helpers.blend_scene("cull", 75, 33), 0.0
    else:
        d, frac = helpers.blend_scene(scene, None, None), 0.0
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v], seg1_fraction=frac)
    assert int(v.flag.item()) == 0
    n_contrib = v.state()["n_contrib"]
    assert (n_contrib > 0).any()
    out = {"n_contrib": _sha(n_contrib)}
    noise, _ = segment_ref.label_plane("draw16", v.W, v.H)      # a seeded per-pixel draw from {0 .. 15, 255}
    for tag, masks in (("contrib", None), ("contrib_masked", [noise < 8])):
        r = dev.contrib([v], masks)
        assert r["hits"].sum() > 0
        out[tag] = {k: _sha(r[k]) for k in KEYS}
    (maps,) = pixel_maps(dev, [v])
    assert (maps["count"] > 0).any()
    out["pixel_maps"] = {p: _sha(maps[p]) for p in PLANES}
    for L in VOTE_LABELS:                                        # (L = 2: the bytes 2 .. 15 of the plane are no label)
        votes, _ = label_votes(dev, [v], [noise], L)
        assert votes.sum() > 0
        out[f"votes_L{L}"] = {"votes": _sha(votes)}
    gl, _ = segment_ref.gaussian_labeling("mod16", dev.P)        # (L < 16: the Gaussians with index mod 16 >= L carry no label)
    for L in RENDER_LABELS:
        ((label, weight),) = label_render(dev, [v], gl, L)
        assert (weight > 0).any()
        out[f"render_L{L}"] = {"label": _sha(label), "weight": _sha(weight)}
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_every_walk_reproduces_the_recorded_bits(scene):
    with open(GOLDEN) as fp:
        want = json.load(fp)[scene]
    got = walk_hashes(scene)
    assert got["n_contrib"] == want["n_contrib"], f"{scene}: the forward's n_contrib differs -- the input state, not the walk"
    assert sorted(got) == sorted(want)
    bad = [(s, a) for s in want if s != "n_contrib" for a in want[s] if got[s].get(a) != want[s][a]]
    assert not bad, f"{scene}: bits differ from the recorded ones in {bad}"
    assert all(sorted(got[s]) == sorted(want[s]) for s in want if s != "n_contrib")
