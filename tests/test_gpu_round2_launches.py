"""The second binning round as separate launches (B3GS_ROUND2_LEGACY: scan2_*, emit_instances<true>, the tile-split passes
with the device-side offset N1) instead of the persistent repair launch.  The switch is read once per process, so the
renders run in their own interpreter; a pair plus one view, so that a scan partner exists.  Bit-identical to one round."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("render", "rendered_depth", "rendered_alpha", "radii")

SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from binocular3dgs_amd import synth
from binocular3dgs_amd.debug import state_views
from binocular3dgs_amd.fused import FusedRasterizer
P, W, H = (int(a) for a in sys.argv[2:5])
model = synth.synth_model(P, seed=P, device="cuda", width=W, height=H, requires_grad=False)
with torch.no_grad():
    model._scaling += 1.0
    model._opacity -= 2.0          # tiles stay open: the second round has work
pairs = synth.synth_view_set(W, H, device="cuda")
bg = torch.tensor([0.2, 0.1, 0.0], device="cuda")
views = [(pairs[0][0], 0), (pairs[0][1], 1), (pairs[1][0], 2)]
res = {}
for frac in (0.0, 0.3):
    fr = FusedRasterizer(model, W, H, num_slots=3, seg1_fraction=frac)
    with torch.no_grad():
        outs = fr.render_batch(views, bg)
    torch.cuda.synchronize()
    assert not fr.overflowed() and int(fr.overflow_flag.item()) == 0
    for v, o in enumerate(outs):
        for k in %(keys)r:
            res["f%%g_v%%d_%%s" %% (frac, v, k)] = o[k].cpu().numpy()
    # N2 of every view (geometry header word 2): the instances the second round emitted.  (repair_rate() counts inside the
    # persistent launch only, which this process does not run.)
    res["n2_%%g" %% frac] = np.array([int(state_views(P, W, H, fr.capacity, s.geom, s.binning, s.img)["counts"][2]) for s in fr.slots])
np.savez(sys.argv[1], **res)
"""


@pytest.mark.parametrize("P,W,H", [(12289, 272, 16), (9000, 208, 144)])
def test_round2_as_separate_launches_equals_one_round(tmp_path, P, W, H):
    env = dict(os.environ)
    env["B3GS_ROUND2_LEGACY"] = "1"
    out = tmp_path / "round2.npz"
    r = subprocess.run([sys.executable, "-c", SNIPPET % {"root": ROOT, "keys": KEYS}, str(out), str(P), str(W), str(H)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    print(f"P={P} {W}x{H}: N2 per view, one round {got['n2_0'].tolist()}, two rounds {got['n2_0.3'].tolist()}")
    assert not got["n2_0"].any() and got["n2_0.3"].sum() > 0, "the second round must have had work"
    for v in range(3):
        for k in KEYS:
            a, b = got[f"f0.3_v{v}_{k}"], got[f"f0_v{v}_{k}"]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (v, k)
