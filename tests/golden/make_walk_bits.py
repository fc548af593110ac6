#!/usr/bin/env python
"""Writes tests/golden/walk_bits.json: the SHA-256 of every output of the four second walks of a forward's tile lists
(contribution, pixel maps, label votes, label render) on the scenes and settings of tests/test_gpu_walk_bits.py, plus the hash
of each forward's n_contrib.  Needs the GPU and the built library; run from the repository root:

    python tests/golden/make_walk_bits.py [output.json]

The file was written ONCE, on the commit before csrc/tile_walk.h, and is what the refactored walk is held to.  Running this on
a later commit only restates what that commit computes: a differing hash is a changed walk, not a stale fixture.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import test_gpu_walk_bits as wb  # noqa: E402


def main(argv):
    path = argv[0] if argv else wb.GOLDEN
    res = {scene: wb.walk_hashes(scene) for scene in wb.SCENES}
    with open(path, "w") as fp:
        json.dump(res, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(f"{path}: {len(res)} scenes, {sum(len(v) for r in res.values() for v in r.values() if isinstance(v, dict))} hashes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
