"""Shared scene builders for the tests (seeded, CPU tensors)."""
import math

import numpy as np
import torch

from binocular3dgs_amd import synth
from binocular3dgs_amd.camera import Camera, look_at_orbit


def small_scene(P=400, W=64, H=48, seed=0, K=4, sh_degree=1, fovx_deg=60.0, yaw=5.0, scale_mu=0.06, near_frac=0.0):
    """Random Gaussians in front of a slightly rotated camera; activated parameters (what the
    rasterizer receives).  near_frac of the points are pushed to / behind the near plane."""
    p = synth.synth_gaussians(P, seed, W, H, fovx_deg, K)
    g = torch.Generator().manual_seed(seed + 77)
    scaling = math.log(scale_mu) + 0.6 * torch.randn(P, 3, generator=g)
    xyz = p["xyz"].clone()
    if near_frac > 0:
        n = int(P * near_frac)
        xyz[:n, 2] = 0.4 * torch.rand(n, generator=g) - 0.1
    fovx = math.radians(fovx_deg)
    fovy = synth.fovy_from(fovx, W, H)
    R, T = look_at_orbit(yaw)
    cam = Camera(R, T, fovx, fovy, W, H)
    d = dict(
        means3D=xyz, opacities=torch.sigmoid(p["opacity"]), scales=torch.exp(scaling),
        rotations=torch.nn.functional.normalize(p["rotation"]),
        shs=torch.cat([p["features_dc"], p["features_rest"]], 1),
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
        bg=torch.tensor([0.1, 0.2, 0.3]), W=W, H=H, tanfovx=math.tan(fovx / 2), tanfovy=math.tan(fovy / 2),
        sh_degree=sh_degree)
    return d, cam


SH_C0 = 0.28209479177387814

# Per-row gradient criterion (row_err / row_failures below).  The bound is NOT taken from the kernels: it is 10x the
# largest 99th percentile of row_err between render_dense(dtype=float32) and render_dense(dtype=float64) -- the
# reference against itself, the float64 run's rects and robust pixel gradients (FRAGILE_MARGIN) given to both -- over the
# six gradient tensors, every configuration the tests use (edge_scene seeds 0 and 1; (K, degree) = (16,0), (16,1), (16,2),
# (16,3), (9,2) at scale_modifier 0.8; the two-camera placement at modifier 1, degrees 2 and 3, per camera).  The factor 10
# leaves room for fp32 atomics in another order and an exp2-based exp.  Measured (99th percentile / maximum of row_err
# over the touched rows), (K, degree) = (16, 3):
#                seed 0 (713 touched)     seed 1 (725 touched)
#   means3D      8.9e-6 / 4.1e-5          1.1e-5 / 7.7e-5
#   opacities    7.7e-6 / 1.7e-5          1.1e-5 / 3.1e-5
#   scales       9.7e-6 / 2.2e-5          6.7e-6 / 1.8e-5
#   rotations    7.1e-6 / 2.8e-5          8.0e-6 / 2.1e-5
#   shs          5.0e-6 / 9.4e-6          4.9e-6 / 8.5e-6
#   means2D      1.0e-5 / 3.8e-5          1.3e-5 / 7.1e-5
# Largest 99th percentile over all configurations: 1.56e-5 (largest single row: 2.6e-4, rotations, seed 0, (9, 2))
# -> bound 1.5e-4.  (Without the robust pixel gradients one flipped 1/255 decision in ONE pixel of one two-camera case
# lifted the 99th percentile of that case to 4.6e-4.)
ROW_BOUND = 1.5e-4
# ... and how many rows may exceed it: 0.5 % of the touched rows of a tensor (2 if that is more), 2 % of the rows of a
# stratum (1 if that is more).  The reference against itself: at most 1 row of ~710 above the bound.
ROW_FRAC_ALL, ROW_MIN_ALL = 0.005, 2
ROW_FRAC_STRATUM, ROW_MIN_STRATUM = 0.02, 1


def edge_scene(P=768, W=80, H=48, seed=0, K=16, sh_degree=3, place_cams=None):
    """small_scene(scale_mu=0.08) with the branches of the per-Gaussian chain rule populated on purpose.  Returns
    (d, cam, built): d and cam as small_scene does (d gains scale_modifier = 0.8), built = {"A", "B"}: boolean masks
    of the Gaussians placed below.  WHICH branch a Gaussian takes is decided by the float64 reference: edge_strata().

      A  the first P//4: outside the 1.3 tan(fov/2) limit of the EWA Jacobian -- a third in x only, a third in y only,
         a third in both (|x/z| resp. |y/z| in [1.35, 1.6] tan(fov/2), random signs, the other axis within 0.9 of the
         frustum), z in [2, 6], scales 0.25 z exp(0.3 N(0,1)) so that the splat reaches the image, opacity in
         [0.03, 0.15] so that it does not hide the scene.  place_cams: cameras (same intrinsics) to place them for,
         in turn; default: the scene's own camera.
      B  the next P//4: one, two, three or three channels (in turn) of the DC row lowered by [0.3, 0.6] / SH_C0: colour
         channels clamped at 0.
      everywhere: higher-order SH of real size (0.3 N(0,1)), non-unit quaternions (length scaled by U[0.5, 2]: the
      standard mode takes q as given, the RAW mode normalises)."""
    d, cam = small_scene(P=P, W=W, H=H, seed=seed, K=K, sh_degree=sh_degree, scale_mu=0.08)
    g = torch.Generator().manual_seed(seed + 4242)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    N = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    nA = P // 4
    cams = list(place_cams) if place_cams else [cam]
    j = torch.arange(nA)
    which_cam, kind = j % len(cams), (j // len(cams)) % 3          # kind 0: x only, 1: y only, 2: both
    z = 2.0 + 4.0 * U(nA)
    out = (1.35 + 0.25 * U(nA, 2)) * torch.where(U(nA, 2) < 0.5, -1.0, 1.0)
    inside = 0.9 * (2.0 * U(nA, 2) - 1.0)
    rx = torch.where(kind != 1, out[:, 0], inside[:, 0]) * d["tanfovx"]
    ry = torch.where(kind != 0, out[:, 1], inside[:, 1]) * d["tanfovy"]
    pv = torch.stack([rx * z, ry * z, z], 1)
    means, scales, opac = d["means3D"].clone(), d["scales"].clone(), d["opacities"].clone()
    for c, cm in enumerate(cams):
        V = cm.world_view_transform.detach().cpu().double()       # row vectors: view = [x y z 1] @ V
        world = (pv - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
        sel = which_cam == c
        means[:nA][sel] = world[sel].float()
    scales[:nA] = (0.25 * z[:, None] * torch.exp(0.3 * N(nA, 3))).float()
    opac[:nA] = (0.03 + 0.12 * U(nA, 1)).float().reshape(opac[:nA].shape)
    shs = d["shs"].clone()
    if K > 1:
        shs[:, 1:] = (0.3 * N(P, K - 1, 3)).float()
    nch = torch.tensor([1, 2, 3, 3])[torch.arange(nA) % 4]         # how many channels of a B row are lowered
    rank = torch.argsort(U(nA, 3), dim=1)                          # ... and which: a random permutation per row
    lower = (0.3 + 0.3 * U(nA, 3)) / SH_C0 * (rank < nch[:, None])
    shs[nA:2 * nA, 0] -= lower.float()
    rot = d["rotations"] * (0.5 + 1.5 * U(P, 1)).float()
    d.update(means3D=means, scales=scales, opacities=opac, shs=shs, rotations=rot, scale_modifier=0.8)
    built = {"A": torch.arange(P) < nA, "B": (torch.arange(P) >= nA) & (torch.arange(P) < 2 * nA)}
    return d, cam, built


def edge_strata(d, viewmatrix=None, campos=None, sh_degree=None):
    """The branch every Gaussian takes, by the float64 reference's own rules (oracle/dense_torch.py): boolean numpy
    masks clamp_x / clamp_y / clamp_xy (view-space x/z, y/z past 1.3 tan(fov/2): in x only, y only, both) and
    ch1 / ch2 / ch3 (exactly one, two, three colour channels clamped at 0).  Another camera of the same intrinsics:
    pass its viewmatrix and campos."""
    from oracle import dense_torch
    V = (d["viewmatrix"] if viewmatrix is None else viewmatrix).detach().cpu().double().reshape(4, 4)
    cp = (d["campos"] if campos is None else campos).detach().cpu().double().reshape(3)
    m = d["means3D"].detach().cpu().double()
    pv = torch.cat([m, torch.ones(len(m), 1, dtype=torch.float64)], 1) @ V
    cx = (pv[:, 0] / pv[:, 2]).abs() > 1.3 * d["tanfovx"]
    cy = (pv[:, 1] / pv[:, 2]).abs() > 1.3 * d["tanfovy"]
    dirs = m - cp
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    deg = d["sh_degree"] if sh_degree is None else sh_degree
    col = dense_torch._sh_rgb(deg, d["shs"].detach().cpu().double(), dirs) + 0.5
    n = (col < 0).sum(1)
    out = dict(clamp_x=cx & ~cy, clamp_y=cy & ~cx, clamp_xy=cx & cy, ch1=n == 1, ch2=n == 2, ch3=n == 3)
    out = {k: v.numpy() for k, v in out.items()}
    out["colour"] = col.numpy()
    return out


STRATA = ("clamp_x", "clamp_y", "clamp_xy", "ch1", "ch2", "ch3")


def strata_population(strata, touched, minimum=20, minimum_ch3=3):
    """{stratum: touched Gaussians in it}; asserts the floor every test relies on (a later change to the builder must
    not empty a stratum unnoticed)."""
    pop = {k: int((strata[k] & touched).sum()) for k in STRATA}
    for k, n in pop.items():
        assert n >= (minimum_ch3 if k == "ch3" else minimum), f"stratum {k} holds {n} touched Gaussians: {pop}"
    return pop


def row_err(got, ref, touched):
    """For each touched row i: |got_i - ref_i| / (|ref_i| + s), s = the median row norm of `ref` over the touched rows.
    A row is touched when the reference's opacity gradient is non-zero.  (Bound and allowance: ROW_BOUND above.)"""
    ref = np.asarray(ref, dtype=np.float64)
    ref = ref.reshape(ref.shape[0], -1)[touched]
    got = np.asarray(got, dtype=np.float64).reshape(-1, ref.shape[1])[touched]
    n = np.linalg.norm(ref, axis=1)
    s = float(np.median(n)) if len(n) else 0.0
    return np.linalg.norm(got - ref, axis=1) / np.maximum(n + s, 1e-300)


def row_failures(got, ref, touched, strata=None, bound=None, names=STRATA):
    """The per-row criterion: -> [(where, rows above the bound, rows, allowed)] for the whole tensor ("all") and each
    stratum that breaks its allowance; empty = passed."""
    bound = ROW_BOUND if bound is None else bound
    err = row_err(got, ref, touched)
    over = err > bound
    allowed = max(int(ROW_FRAC_ALL * len(err)), ROW_MIN_ALL)
    bad = [("all", int(over.sum()), len(err), allowed)] if int(over.sum()) > allowed else []
    for k in (names if strata is not None else ()):
        m = strata[k][touched]
        allowed = max(int(ROW_FRAC_STRATUM * int(m.sum())), ROW_MIN_STRATUM)
        if int(over[m].sum()) > allowed:
            bad.append((k, int(over[m].sum()), int(m.sum()), allowed))
    return bad


# Pixels at which the float64 reference comes within this relative distance of another decision (an alpha at 1/255, a
# running transmittance at 1e-4: render_dense's `margin`) get a zero upstream gradient in the gradient tests, on both
# sides: a float32 implementation may decide otherwise there, and ONE such pixel moves the rows of every Gaussian it
# holds (measured: reference float32 against float64, one flipped pixel of 3840 put 16 of 719 opacity rows above
# ROW_BOUND).  float32 error of an alpha: its exponent reaches ln 255 = 5.5 and carries a few ulps of the conic, whose
# determinant cancels -> up to ~5e-5 relative; 3e-4 leaves a factor 6 and excludes ~1 % of the pixels (40 of 3840).
FRAGILE_MARGIN = 3e-4


def robust_pixel_grads(out, pixel_grads):
    """pixel_grads with the pixels zeroed whose decisions are fragile in the reference forward `out` (FRAGILE_MARGIN)."""
    ok = (out["margin"] >= FRAGILE_MARGIN).to(torch.float64)
    return tuple(t.double() * ok for t in pixel_grads)


def dense_grads(d, rect, pixel_grads, names=("means3D", "opacities", "scales", "rotations", "shs"), dtype=torch.float64,
                robust=True):
    """render_dense of the scene dict `d` with `rect` imposed, and autograd gradients of
    sum(colour gc) + sum(depth gd) + sum(alpha ga) w.r.t. d[names] and the pixel positions; robust: (gc, gd, ga) go
    through robust_pixel_grads first.
    -> (outputs, {name: gradient [P, ...], "means2D": [P, 2] in the units of means2D.grad}, the (gc, gd, ga) used)."""
    from oracle import dense_torch
    P = d["means3D"].shape[0]
    leaf = {k: d[k].to(dtype).clone().requires_grad_(True) for k in names}
    off = torch.zeros(P, 2, dtype=dtype, requires_grad=True)
    out = dense_torch.render_dense(**{**d, **leaf}, rect=rect, pix_offset=off, dtype=dtype)
    pixel_grads = robust_pixel_grads(out, pixel_grads) if robust else tuple(t.double() for t in pixel_grads)
    gc, gd, ga = (t.to(dtype) for t in pixel_grads)
    ((out["color"] * gc).sum() + (out["depth"] * gd).sum() + (out["alpha"] * ga).sum()).backward()
    grads = {k: v.grad.reshape(P, -1).double().numpy() for k, v in leaf.items()}
    grads["means2D"] = (off.grad.double() * torch.tensor([0.5 * d["W"], 0.5 * d["H"]], dtype=torch.float64)).numpy()
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}, grads, pixel_grads


def oracle_kwargs(d, **over):
    kw = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    kw.update(over)
    return kw


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# Scenes of the blend edge tests (tests/test_blend_ref_cpu.py, tests/test_gpu_blend_edges.py): flat splats placed in
# PIXEL units in front of a camera at the origin looking down +z, so that a list length, a saturation point or a footprint
# edge can be put where the blend kernels change path.  What a scene really holds is decided by the float64 reference
# (tests/blend_ref.py) on the projected records, and asserted there.
# ---------------------------------------------------------------------------------------------------------------------
BLEND_FOVX = math.radians(60.0)
BLEND_BG = (0.1, 0.2, 0.3)
STACK_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
LADDERS = {"ladder_b": (-0.535, -0.165, 13.064, 0.297), "ladder_c": (0.831, -1.665, 13.374, 0.281)}   # x, y, sigma, opacity


def splat_scene(W, H, x, y, sig_a, sig_b, theta, opacity, colour, z):
    """Scene dict (small_scene's keys, activated parameters, sh_degree 0) of flat splats: centre (x, y) in pixels, standard
    deviations sig_a, sig_b in pixels along / across the direction theta, at view depth z.  (The projection adds its 0.3
    pixel^2 dilation and, off axis, a little shear.)"""
    n = len(x)
    f64 = lambda a: np.broadcast_to(np.asarray(a, np.float64), (n,)).copy()  # noqa: E731
    x, y, sig_a, sig_b, theta, opacity, z = (f64(a) for a in (x, y, sig_a, sig_b, theta, opacity, z))
    fovy = synth.fovy_from(BLEND_FOVX, W, H)
    tx, ty = math.tan(BLEND_FOVX / 2), math.tan(fovy / 2)
    fx = W / (2 * tx)
    X = z * tx * ((2 * x + 1) / W - 1)
    Y = z * ty * ((2 * y + 1) / H - 1)
    scales = np.stack([sig_a * z / fx, sig_b * z / fx, 1e-4 * z / fx], 1)
    rot = np.stack([np.cos(theta / 2), np.zeros(n), np.zeros(n), np.sin(theta / 2)], 1)
    cam = Camera(*look_at_orbit(0.0), BLEND_FOVX, fovy, W, H)
    shs = (np.asarray(colour, np.float64).reshape(n, 1, 3) - 0.5) / SH_C0
    t32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)  # noqa: E731
    return dict(means3D=t32(np.stack([X, Y, z], 1)), opacities=t32(opacity).reshape(n, 1), scales=t32(scales),
                rotations=t32(rot), shs=t32(shs), viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                campos=cam.camera_center, bg=torch.tensor(BLEND_BG), W=W, H=H, tanfovx=tx, tanfovy=ty, sh_degree=0)


def _stack(rng, L, cx, cy, sigma, opacity, z0):
    return dict(x=np.full(L, cx), y=np.full(L, cy), sig_a=np.full(L, sigma), sig_b=np.full(L, sigma), theta=np.zeros(L),
                opacity=np.full(L, opacity), colour=rng.uniform(0.05, 0.95, (L, 3)), z=z0 + 0.004 * np.arange(L))


def _cat(*parts):
    return {k: np.concatenate([np.asarray(p[k], np.float64) for p in parts]) for k in parts[0]}


def _cull_field(rng, W, H, n=600):
    """Small and elongated splats on and around quadrant / tile corners and edges: a quarter barely visible (opacity 1.1/255
    to 2/255), a fifth opaque and centred on a pixel (alpha clamped at 0.99 there), aspect up to 20:1, all rotations."""
    kind = rng.uniform(size=n)
    gxs, gys = np.arange(0, W + 8, 8), np.arange(0, H + 8, 8)
    x = rng.choice(gxs, n) - 0.5 + rng.normal(0, 2.0, n)
    y = rng.choice(gys, n) - 0.5 + rng.normal(0, 2.0, n)
    edge = rng.uniform(size=n) < 0.4          # on an edge between two corners
    y = np.where(edge & (rng.uniform(size=n) < 0.5), rng.uniform(-2, H + 2, n), y)
    x = np.where(edge & (rng.uniform(size=n) < 0.5), rng.uniform(-2, W + 2, n), x)
    long_ = np.exp(rng.uniform(math.log(0.8), math.log(7.0), n))
    short = long_ / rng.uniform(1.0, 20.0, n)
    op = rng.uniform(0.02, 0.6, n)
    op = np.where(kind < 0.25, rng.uniform(1.1 / 255, 2.0 / 255, n), op)
    # faint ones: wide enough to be live over several pixels
    long_ = np.where(kind < 0.25, np.maximum(long_, 2.0), long_)
    opaque = kind > 0.8
    op = np.where(opaque, 0.9999, op)
    x = np.where(opaque, np.round(x) + rng.normal(0, 0.05, n), x)
    y = np.where(opaque, np.round(y) + rng.normal(0, 0.05, n), y)
    long_ = np.where(opaque, rng.uniform(1.5, 3.0, n), long_)
    short = np.where(opaque, long_ * rng.uniform(0.6, 1.0, n), short)
    return dict(x=x, y=y, sig_a=long_, sig_b=short, theta=rng.uniform(0, math.pi, n), opacity=op,
                colour=rng.uniform(0.05, 0.95, (n, 3)), z=rng.uniform(2.0, 6.0, n))


def blend_scene(name, W=None, H=None):
    """The scenes of the blend edge tests, by name -> scene dict (splat_scene):
      stack<L>   64 x 16: L identical wide splats (sigma 10, opacity 0.009) on the centre of tile 0: every pixel of the tile
                 blends all L.  (By the reference's 3-sigma rectangle such a footprint also reaches tiles 1 and 2, which hold
                 the same list with fewer live pixels; tile 3 stays empty.  Only tile 0 is the designed stack -- n_contrib = L
                 at every pixel, the backward starts exactly at the list's end; in tiles 1 and 2 n_contrib is mixed.)
      ladder_b / ladder_c   64 x 16: 300 identical splats (LADDERS: sigma ~13, opacity ~0.29) centred next to the corner of
                 tile 0: alpha falls off smoothly across tiles 0-2, pixels saturate at list positions ~30-290; the quadrants
                 of tile 0 finish at ~37, 67, 68 and 118 (tile 0 is done before its second 256-entry chunk).  The centres were
                 searched so that the two scenes together hold pixels saturating at every position 62..66 and 254..258.
      cull       the cull field (default 96 x 64; any W, H)
      wide       64 x 16: stack65 behind one splat of sigma 40 over every tile"""
    rng = np.random.RandomState(abs(hash_name(name)) % (2 ** 31))
    if name.startswith("stack"):
        W, H = 64, 16
        spec = _stack(rng, int(name[5:]), 7.5, 7.5, 10.0, 0.009, 2.0)
    elif name in ("ladder_b", "ladder_c"):
        W, H = 64, 16
        spec = _stack(rng, 300, *LADDERS[name], 2.0)
    elif name.startswith("cull"):          # ("cull" + anything: another draw of the field)
        W, H = W or 96, H or 64
        spec = _cull_field(rng, W, H)
    elif name == "wide":
        W, H = 64, 16
        wide = dict(x=[31.5], y=[7.5], sig_a=[40.0], sig_b=[40.0], theta=[0.0], opacity=[0.3], colour=[[0.8, 0.3, 0.5]], z=[1.5])
        spec = _cat(wide, _stack(rng, 65, 7.5, 7.5, 10.0, 0.009, 2.0))
    else:
        raise KeyError(name)
    return splat_scene(W, H, **spec)


def hash_name(name):
    """A seed from a scene name that does not depend on the interpreter's string hashing."""
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) * 2654435761 % (2 ** 31)


def oracle_records(st):
    """[P, 10] float32 records (x, y, conic xx, xy, yy, opacity, r, g, b, depth) of an oracle.tile_ref State."""
    return np.concatenate([st.means2D, st.conic_opacity[:, :3], st.conic_opacity[:, 3:4], st.rgb, st.depths[:, None]],
                          1).astype(np.float32)


# Bounds of the blend edge tests: 10 x the largest 99th percentile of float32 blend_ref against float64 blend_ref over
# BLEND_CASES (tests/test_blend_ref_cpu.py measures and pins them; the figures are in tests/test_gpu_blend_edges.py).
# images: |x - ref| <= bound (1 + |ref|); final_T: absolute; rows: row_err.  The image measurement asks for 3.3e-5
# (stack513); the bound stays at the existing contract of 3e-5.
BLEND_IMG_BOUND, BLEND_T_BOUND, BLEND_ROW_BOUND = 3.0e-5, 2.1e-5, 1.1e-4
BLEND_IMG_CONTRACT = 3.0e-5
BLEND_CASES = tuple(("stack%d" % L, None, None) for L in STACK_LENGTHS) + (
    ("ladder_b", None, None), ("ladder_c", None, None), ("cull", 96, 64), ("cull", 72, 41), ("cull", 75, 33), ("wide", None, None))
BLEND_STRATA = ("cullable", "corner", "seam", "sat_at_seam", "late", "clamped", "faint")
# floors of the populations a scene must hold (Gaussians per stratum, after fragility); pairs: (tile, quadrant, Gaussian)
BLEND_FLOORS = {"cull": dict(cullable=150, corner=100, clamped=50, faint=20, seam=10, sat_at_seam=20),
                "ladder_b": dict(corner=20, seam=6, sat_at_seam=50, late=3), "ladder_c": dict(corner=20, seam=6, sat_at_seam=50, late=3)}
BLEND_PAIR_FLOORS = {"cull": dict(cullable=200, corner=100)}


def blend_pixel_grads(W, H, seed=3):
    """Seeded float32 pixel gradients (colour [3,H,W], depth, alpha [H,W]) of the blend edge tests."""
    rng = np.random.RandomState(seed)
    hw = W * H
    return ((rng.normal(size=(3, H, W)) / (3 * hw)).astype(np.float32), (rng.normal(size=(H, W)) / hw).astype(np.float32),
            (rng.normal(size=(H, W)) / hw).astype(np.float32))


def blend_populations(name, st, masks, lost, pr, tight=False):
    """Assert what the tests rely on in scene `name` (a float64 blend_ref State and its strata); -> figures to print.
    tight: the lists are those of tight binning -- shorter, so the floors tied to a list POSITION (seam, sat_at_seam) and
    the ladders' designed finish positions do not apply; the footprint strata do."""
    from blend_ref import SEAMS
    key = "cull" if name.startswith("cull") else name
    pop = {k: (int(masks[k].sum()), int(lost[k].sum())) for k in BLEND_STRATA}
    for k, (n, gone) in pop.items():
        assert gone <= 0.1 * n, f"{name}: stratum {k} loses {gone} of {n} members to fragility"
    for k, floor in BLEND_FLOORS.get(key, {}).items():
        if tight and k in ("seam", "sat_at_seam"):
            continue
        assert pop[k][0] - pop[k][1] >= floor, f"{name}: stratum {k} holds {pop[k]} (floor {floor})"
    npairs = dict(cullable=int((pr["reach"] & pr["walked"] & (pr["n_alive"] == 0) & ~pr["near"]).sum()),
                  corner=int(((pr["n_blend"] >= 1) & (pr["n_blend"] <= 3) & (pr["n_solid"] >= 1)).sum()))
    for k, floor in BLEND_PAIR_FLOORS.get(key, {}).items():
        assert npairs[k] >= floor, f"{name}: {npairs[k]} {k} pairs (floor {floor})"
    W, H = st.W, st.H
    if name.startswith("stack"):
        L = int(name[5:])
        assert (st.n_contrib[:16, :16] == L).all() and st.work[0] == L, "every pixel of tile 0 blends the whole stack"
        assert len(st.ids[3]) == 0, "tile 3 is empty"
        assert pop["seam"][0] == sum(s < L for s in SEAMS)
    if name.startswith("ladder") and not tight:
        fin = {t: sorted(set(pr["finish"][(pr["tile"] == t)].tolist())) for t in range(3)}
        assert max(fin[0]) - min(fin[0]) > 64, f"a quadrant of tile 0 finishes more than 64 entries before another: {fin[0]}"
        assert max(fin[0]) < 256 < len(st.ids[0]), "tile 0 finishes before its last chunk"
        if name == "ladder_b":   # quadrant finish positions of every residue mod 4 (the forward looks every 4th candidate)
            assert {f % 4 for f in fin[0] + fin[1] + fin[2] if 0 < f < len(st.ids[0])} == {0, 1, 2, 3}, fin
        # the saturating entry is not blended, final_T is the value before it
        sat = st.sat_pos >= 0
        assert sat.any() and (st.n_contrib[sat] <= st.sat_pos[sat]).all() and (st.final_T[sat] >= 1e-4).all()
    if key == "cull" and (W % 16 or H % 16):
        t_out = [(t, q) for t, q, f_ in zip(pr["tile"], pr["quad"], pr["finish"]) if f_ == 0 and st.work[t] > 0]
        assert len(t_out) > 0, "a tile with work holds a quadrant wholly outside the image"
    if name == "wide":
        wide = (pr["gid"] == 0) & (pr["n_blend"] > 0)
        assert wide.sum() == 16, "the wide splat is blended by every quadrant of every tile"
    return pop, npairs


BLEND_BATCH_SIZES = ((80, 48), (72, 41), (33, 17))
BLEND_BATCH_FLOORS = dict(touched=400, cullable=100, corner=100)


def blend_batch_scenes(name="cull_batch7", sizes=BLEND_BATCH_SIZES):
    """One cull field (built for the first size) seen by cameras of several resolutions: the views of a batched launch."""
    ds = [blend_scene(name, *sizes[0])]
    for W, H in sizes[1:]:
        e = splat_scene(W, H, [0.0], [0.0], 1.0, 1.0, 0.0, 0.5, [[0.5, 0.5, 0.5]], 2.0)
        d = dict(ds[0])
        d.update({k: e[k] for k in ("viewmatrix", "projmatrix", "campos", "W", "H", "tanfovx", "tanfovy")})
        ds.append(d)
    return ds


# The two-segment scene: P = 4096 + 512, 160 x 16 (ten tiles).  Segment 1 of a two-round forward is the nearest 4096 Gaussians
# of the depth order; most of those sit far outside the image (they take their place in the order and emit no instance), so
# that the number of segment-1 entries per tile -- len1 -- is chosen per tile: (len1, len2) below, narrow splats (sigma 2.1:
# the reference's rectangle stays inside the tile) that leave the corners of their tile untouched, i.e. the tile open.  Tile 9
# holds 30 wide opaque splats of segment 1 that terminate every pixel of it -- no segment 2 may arrive there although ten wide
# splats of segment 2 lie on it -- and spill into tiles 7 and 8, which stay open.  Tile 6 is empty.
TWO_SEG_P, TWO_SEG_K1, TWO_SEG_SIZE = 4096 + 512, 4096, (160, 16)
TWO_SEG_TILES = {0: (64, 20), 1: (70, 30), 2: (128, 10), 3: (100, 70), 4: (0, 12), 5: (256, 40)}
TWO_SEG_OPAQUE = (30, 10)


def two_segment_scene(P=TWO_SEG_P, K1=TWO_SEG_K1):
    """(P, K1) other than the defaults: the same tiles with more filler, so that segment 1 is the nearest K1 of P Gaussians"""
    rng = np.random.RandomState(hash_name("two_segments"))
    W, H = TWO_SEG_SIZE
    parts1, parts2 = [], []
    for t, (n1, n2) in TWO_SEG_TILES.items():
        for n, parts, z0 in ((n1, parts1, 2.0), (n2, parts2, 4.0)):
            if n:
                s = _stack(rng, n, 16 * t + 7.5, 7.5, 2.1, 0.03, z0 + 0.05 * t)
                s["z"] = z0 + 0.05 * t + 1e-4 * np.arange(n)
                parts.append(s)
    for n, parts, z0 in ((TWO_SEG_OPAQUE[0], parts1, 2.9), (TWO_SEG_OPAQUE[1], parts2, 4.9)):
        s = _stack(rng, n, 16 * 9 + 7.5, 7.5, 12.0, 0.9, z0)
        s["z"] = z0 + 1e-4 * np.arange(n)
        parts.append(s)
    n_on1, n_on2 = sum(len(p["x"]) for p in parts1), sum(len(p["x"]) for p in parts2)
    for n, parts, z0 in ((K1 - n_on1, parts1, 1.0), (P - K1 - n_on2, parts2, 6.0)):
        s = _stack(rng, n, -400.0, 7.5, 1.0, 0.5, z0)       # outside the image: a place in the depth order, no instance
        s["z"] = z0 + 1e-4 * np.arange(n)
        parts.append(s)
    return splat_scene(W, H, **_cat(*(parts1 + parts2)))


def two_segment_populations(len1, len2, opaque_tile=9):
    """Assert, from per-tile segment lengths, what the two-segment test relies on."""
    len1, len2 = np.asarray(len1), np.asarray(len2)
    both = (len1 > 0) & (len2 > 0)
    assert (both & (len1 % 64 == 0)).any(), f"no open tile whose len1 sits on a 64-entry word boundary: {len1} {len2}"
    assert (both & (len1 % 64 != 0)).any(), f"no open tile whose len1 falls strictly inside a word: {len1} {len2}"
    assert ((len1 == 0) & (len2 > 0)).any(), "no tile that holds segment 2 only"
    assert len1[opaque_tile] > 0 and len2[opaque_tile] == 0, "the terminated tile must not receive a segment 2"
    assert (both & (len1 + len2 > 256)).any(), "no list that crosses a staged chunk behind the segment switch"


def blend_batch_populations(st, pr, touched):
    """Floors for a view of the batched launch (the smallest, 33 x 17, is 3 x 2 ragged tiles) -> the figures."""
    fig = dict(touched=int(touched.sum()),
               cullable=int((pr["reach"] & pr["walked"] & (pr["n_alive"] == 0) & ~pr["near"]).sum()),
               corner=int(((pr["n_blend"] >= 1) & (pr["n_blend"] <= 3) & (pr["n_solid"] >= 1)).sum()))
    for k, floor in BLEND_BATCH_FLOORS.items():
        assert fig[k] >= floor, f"batch view {st.W}x{st.H}: {k} {fig[k]} (floor {floor})"
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# Scenes of the binning edge tests (tests/test_gpu_binning_edges.py, reference: tests/binning_ref.py): splat_scene under the
# identity view matrix, so that view z IS the stored z and a depth key can be planted as a bit pattern.  A "one-tile" splat
# (sigma 0.5 -> radius 3) sits on a tile centre, a "two-tile" one on the edge between two tiles of a row.  What a scene really
# holds -- N, V, ties, keys, tiles -- is asserted from the device state by the test (the list at the end of this section records what each must hold).
# ---------------------------------------------------------------------------------------------------------------------
KEY27_BASE, KEY27_SPAN = 0x3E4CCCCD, 1 << 27          # float bits of the near plane 0.2f; span of the three-pass depth sort
BIN_SEAM_P = (1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 16384, 16385, 32769)
BIN_N_TARGETS = (4095, 4096, 4097, 16384, 16385, 32769)
BIN_TILE_IMAGES = {"tiles256": (256, 256, 256), "tiles257": (4112, 16, 257), "tiles257_gridx1": (16, 4112, 257),
                   "tiles513": (432, 304, 513), "tiles1": (16, 16, 1)}
BIN_BATCH_SIZES = ((64, 48), (80, 48), (72, 41), (33, 17), (160, 16), (16, 160), (48, 48), (96, 64))


def bits_to_z(bits):
    return np.asarray(bits, np.uint32).view(np.float32).astype(np.float64)


def _bin_spec(rng, W, H, P, z, two=0.15, big=0.02, cull_every=20, tile=None, empty=0.0):
    """P splats on tile centres of a W x H image (`tile`: all on that one), a share `two` across a tile edge, a share `big`
    wide (sigma 12), a share `empty` outside the image (a place in the depth order, no tile); every `cull_every`-th index (from
    7 on) behind the near plane."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    t = rng.randint(0, gx * gy, P) if tile is None else np.broadcast_to(np.asarray(tile), (P,)).copy()
    kind = rng.uniform(size=P)
    x = 16.0 * (t % gx) + 7.5 + np.where((kind < two) & (gx > 1), 8.0, 0.0)
    y = 16.0 * (t // gx) + 7.5
    sig = np.where(kind > 1.0 - big, 12.0, 0.5)
    x = np.where(rng.uniform(size=P) < empty, -400.0, x)
    z = np.array(np.broadcast_to(z, (P,)), np.float64)
    if cull_every:
        z[7::cull_every] = 0.1
    return dict(x=x, y=y, sig_a=sig, sig_b=sig, theta=np.zeros(P), opacity=np.full(P, 0.5), colour=rng.uniform(0.05, 0.95, (P, 3)), z=z)


def binning_scene(name, P=None, W=64, H=48):
    """The scenes of the binning edge tests, by name -> scene dict (splat_scene).
      seam        P splats, random distinct-ish depths in [0.5, 40], 5 % behind the near plane interleaved by index
      ties_one / ties3 / ties_low9 / ties_mid9   the same with one depth, three depths, keys that differ only in their lowest 9
                  bits, only in bits 18-26 of (key - KEY27_BASE)
      span / span_out   keys KEY27_BASE + 1 and KEY27_BASE + 2^27 - 3 among P = 300; span_out adds KEY27_BASE + 2^27 - 2
      count<N>    N - 10 one-tile splats + 5 two-tile ones: N instances
      cover       160 x 160, P = 600: two splats over all 100 tiles at depth ranks 255 and 256, the rest on one tile each
      sparse      P = 5000, 80 % outside the image
      onetile     P = 9000, every instance in tile 5 (40 distinct depths)
      tiles<T>... (BIN_TILE_IMAGES) every tile of the image holds at least two one-tile splats"""
    rng = np.random.RandomState(abs(hash_name(name + str(P))) % (2 ** 31))
    zrand = lambda n: rng.uniform(0.5, 40.0, n).astype(np.float32).astype(np.float64)  # noqa: E731
    if name == "seam":
        spec = _bin_spec(rng, W, H, P, zrand(P))
    elif name.startswith("ties"):
        if name == "ties_one":
            z = np.full(P, 3.25)
        elif name == "ties3":
            z = rng.choice([1.5, 3.25, 7.0], P)
        elif name == "ties_low9":
            z = bits_to_z(((KEY27_BASE + 0x100000) & ~0x1FF) + rng.randint(0, 512, P))
        else:
            z = bits_to_z(KEY27_BASE + 1 + (rng.randint(0, 512, P).astype(np.int64) << 18))
        spec = _bin_spec(rng, W, H, P, z)
    elif name in ("span", "span_out"):
        P = 300
        z = zrand(P)
        z[11], z[12], z[200], z[201] = bits_to_z([KEY27_BASE + 1, KEY27_BASE + KEY27_SPAN - 3] * 2)
        if name == "span_out":
            z[100] = bits_to_z([KEY27_BASE + KEY27_SPAN - 2])[0]
        spec = _bin_spec(rng, W, H, P, z, big=0.0, cull_every=0)
        spec["x"][[11, 12, 100, 200, 201]], spec["y"][[11, 12, 100, 200, 201]] = 31.5, 23.5     # the image centre: four tiles
    elif name.startswith("count"):
        n = int(name[5:])
        P = n - 5
        spec = _bin_spec(rng, W, H, P, zrand(P), two=0.0, big=0.0, cull_every=0)
        spec["x"][100:105] += 8.0 - 16.0 * (spec["x"][100:105] > W - 16)
    elif name == "cover":
        W, H, P = 160, 160, 600
        rank = rng.permutation(P)
        i255, i256 = int(np.nonzero(rank == 255)[0][0]), int(np.nonzero(rank == 256)[0][0])
        spec = _bin_spec(rng, W, H, P, 1.0 + 0.01 * rank, two=0.0, big=0.0, cull_every=0)
        spec["sig_a"][[i255, i256]] = spec["sig_b"][[i255, i256]] = 160.0
    elif name == "sparse":
        P = 5000
        spec = _bin_spec(rng, W, H, P, zrand(P), empty=0.8)
    elif name == "onetile":
        P = 9000
        spec = _bin_spec(rng, W, H, P, rng.choice(zrand(40), P), two=0.0, big=0.0, tile=5)
    elif name in BIN_TILE_IMAGES:
        W, H, T = BIN_TILE_IMAGES[name]
        P = max(2 * T + 3, 40)
        spec = _bin_spec(rng, W, H, P, zrand(P), two=0.0, big=0.0, cull_every=0, tile=rng.permutation(P) % T)
    else:
        raise KeyError(name)
    return splat_scene(W, H, **spec)


def binning_views(d, sizes, shifts=None):
    """The Gaussians of scene d seen by cameras of other image sizes: same view matrix (so the same depth keys), moved by
    shifts[k] = (dx, dz) in the view's own x / z (dz != 0: other keys; a huge dx: nothing on screen)."""
    out = []
    for k, (W, H) in enumerate(sizes):
        e = splat_scene(W, H, [0.0], [0.0], 1.0, 1.0, 0.0, 0.5, [[0.5, 0.5, 0.5]], 2.0)
        v = dict(d)
        v.update({key: e[key] for key in ("viewmatrix", "projmatrix", "campos", "W", "H", "tanfovx", "tanfovy")})
        dx, dz = (0.0, 0.0) if shifts is None else shifts[k]
        if dx or dz:
            vm = e["viewmatrix"].clone()
            vm[3, 0], vm[3, 2] = -dx, dz
            v["viewmatrix"], v["projmatrix"] = vm, vm @ e["projmatrix"]      # (the unmoved view matrix is the identity)
            v["campos"] = torch.tensor([dx, 0.0, -dz])
        out.append(v)
    return out


# What each case of the binning edge tests must hold; the tests assert it from the device state before anything is compared
# (the populate functions of tests/test_gpu_binning_edges.py):
#   "seam": "V < P (5 % culled), N > V (two-tile and wide splats), at most a few tied keys",
#   "ties_one": "one distinct visible key", "ties3": "three distinct visible keys",
#   "ties_low9": "keys equal above bit 9, > 256 distinct", "ties_mid9": "(key - KEY27_BASE) zero outside bits 18-26, > 256 distinct",
#   "span": "min key KEY27_BASE + 1, max key KEY27_BASE + 2^27 - 3, both in the lists", "span_out": "max key KEY27_BASE + 2^27 - 2",
#   "count<N>": "N instances, five Gaussians of two tiles", "cover": "two Gaussians of 100 tiles at depth ranks 255 and 256",
#   "sparse": "V <= 0.25 P", "onetile": "one distinct tile id, N > 8192", "tiles<T>": "exactly T distinct tile ids",


# ---------------------------------------------------------------------------------------------------------------------
# Scenes of the projection edge tests (tests/test_projection_ref_cpu.py, tests/test_gpu_projection_edges.py; reference:
# tests/projection_ref.py): edge_scene with the branches of the forward projection populated on purpose.  WHICH stratum a
# Gaussian belongs to in a view is decided by the float64 reference (projection_strata), never by construction alone.
# ---------------------------------------------------------------------------------------------------------------------
PROJ_P = 829                          # no multiple of 64 or 256; three 256-thread blocks and a tail
PROJ_SIZES = ((80, 48), (75, 33), (33, 17))
PROJ_SH_CONFIGS = ((1, 0), (4, 0), (4, 1), (9, 2), (16, 1), (16, 3))          # (stored K, active degree)
PROJ_NEAR_Z = tuple(float(v) for v in (np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(0)), np.nextafter(np.float32(0.2), np.float32(1)),
                                       np.float32(0.2) * np.float32(1 - 1e-3), np.float32(0.2) * np.float32(1 + 1e-3)))
PROJ_CAM_B_TZ = 2.0 ** -6             # camera B: identity rotation, this translation along z: view z = z_world + 2^-6 exactly
PROJ_FAINT_BANDS = ((0.0030, 0.0039), (0.0039, 1.0 / 255), (1.0 / 255, 0.0040), (0.0040, 0.006))
PROJ_STRATA = ("clamp_x", "clamp_y", "clamp_xy", "edge_l", "edge_r", "edge_t", "edge_b", "align", "faint", "solid", "needle", "speck",
               "sheet", "ch1", "ch2", "ch3", "quat")
PROJ_FLOORS = dict(align=10)          # non-fragile members; every other stratum: 20 (near: 6 per value, faint: 8 per band)
# Bounds of the float record words against the float64 reference: 10 x the largest 99th percentile of oracle/tile_ref.c
# (float32) against tests/projection_ref.py over every scene, camera, size and SH configuration above
# (tests/test_projection_ref_cpu.py measures and pins them; the table is in tests/test_gpu_projection_edges.py).
# |err| / (1 + |x|); the conic against the largest conic entry of its Gaussian.
PROJ_POS_BOUND, PROJ_CONIC_BOUND, PROJ_RGB_BOUND, PROJ_DEPTH_BOUND = 1.5e-5, 4.1e-5, 1.2e-6, 8.4e-7


def projection_cameras(W, H):
    """{"A": the yaw-8 camera of synth_view_set, "A2": its binocular partner, "B": the axis-aligned near-plane camera}"""
    cam, partner, _t = synth.synth_view_set(W, H)[1]
    fovx = math.radians(60.0)
    b = Camera(np.eye(3), np.array([0.0, 0.0, PROJ_CAM_B_TZ]), fovx, synth.fovy_from(fovx, W, H), W, H)
    return {"A": cam, "A2": partner, "B": b}


def with_camera(d, cam):
    """scene dict d seen by another camera (its own size and field of view)"""
    v = dict(d)
    v.update(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
             W=cam.image_width, H=cam.image_height, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2))
    return v


def projection_scene(W=80, H=48, K=16, sh_degree=3, seed=0):
    """edge_scene(P = 829, scale_modifier 0.8, stratum A placed for camera A and its partner in turn) with further Gaussians
    planted among its last half, then all rows permuted (i -> 367 i mod 829) so that every wave holds several kinds.
    -> (d, cams, planted): d as edge_scene's (camera A; with_camera for the others), cams = projection_cameras,
    planted = {name: indices} of what was placed where (the strata are decided by projection_strata).  Placed in pixel units
    of camera A at size W x H; near: on camera B's axis at the five view depths PROJ_NEAR_Z."""
    cams = projection_cameras(W, H)
    d, _cam, _built = edge_scene(P=PROJ_P, W=W, H=H, seed=seed, K=K, sh_degree=sh_degree, place_cams=[cams["A"], cams["A2"]])
    d = with_camera(d, cams["A"])
    P, nA = PROJ_P, PROJ_P // 4
    rng = np.random.RandomState(1000 * seed + W)
    tx, ty = d["tanfovx"], d["tanfovy"]
    fx = W / (2 * tx)
    means, scales, opac = d["means3D"].double().numpy().copy(), d["scales"].double().numpy().copy(), d["opacities"].double().numpy().reshape(-1).copy()
    rot, shs = d["rotations"].double().numpy().copy(), d["shs"].double().numpy().copy()
    Va = cams["A"].world_view_transform.double().numpy()
    to_world = lambda pv: (pv - Va[3, :3]) @ np.linalg.inv(Va[:3, :3])  # noqa: E731
    pix = lambda px, py, z: np.stack([z * tx * ((2 * px + 1) / W - 1), z * ty * ((2 * py + 1) / H - 1), z], 1)  # noqa: E731
    sigma = lambda s_px, z: s_px * z / (fx * 0.8)  # noqa: E731      (world scale of a splat of s_px pixels at depth z)
    nxt = [2 * nA]
    planted = {}

    def take(name, n):
        idx = np.arange(nxt[0], nxt[0] + n)
        nxt[0] += n
        assert nxt[0] <= P
        planted[name] = idx
        return idx

    # three channels lowered for good in a part of stratum B (edge_scene lowers them by chance)
    b3 = nA + np.arange(3, nA, 4)[:40]
    shs[b3, 0] -= 1.2 / SH_C0
    # near the clamp limit: |x/z| (|y/z|) within 2 % of 1.3 tan
    i = take("clamp_near", 32)
    z = rng.uniform(2, 6, 32)
    f = 1.3 * (1 + rng.uniform(-0.02, 0.02, (32, 2))) * rng.choice([-1.0, 1.0], (32, 2))
    inner = rng.uniform(-0.9, 0.9, (32, 2))
    kind = np.arange(32) % 3
    means[i] = to_world(np.stack([np.where(kind != 1, f[:, 0], inner[:, 0]) * tx * z, np.where(kind != 0, f[:, 1], inner[:, 1]) * ty * z, z], 1))
    scales[i] = (0.25 * z * np.exp(0.3 * rng.normal(size=32)))[:, None] * np.ones(3)
    opac[i] = rng.uniform(0.03, 0.15, 32)
    # centre outside the image on one side; every second one wide enough to reach in
    for name in ("edge_l", "edge_r", "edge_t", "edge_b"):
        n = 28
        i = take(name, n)
        z = rng.uniform(2, 6, n)
        span, other = (W, H) if name[-1] in "lr" else (H, W)
        dist = rng.uniform(1.0, max(2.0, 0.12 * span), n)            # (beyond 0.15 of the image the Jacobian clamp sets in)
        reach = np.arange(n) % 2 == 0
        beyond = 16 * ((span + 15) // 16) - span if name[-1] in "rb" else 0      # the partial last tile still belongs to the grid
        s_px = np.where(reach, (dist + rng.uniform(2, 12, n)) / 3.0, 0.05)
        dist = np.where(reach, dist, dist + beyond + 3.5)
        along = rng.uniform(0, other - 1, n)
        c = -0.5 - dist if name[-1] in "lt" else span - 0.5 + dist
        means[i] = to_world(pix(c, along, z) if name[-1] in "lr" else pix(along, c, z))
        scales[i] = sigma(s_px, z)[:, None] * np.ones(3)
        opac[i] = rng.uniform(0.2, 0.8, n)
    # faint: four bands of the activated opacity around the 0.0039 gate and 1/255
    i = take("faint", 40)
    band = np.arange(40) % 4
    lo, hi = np.array(PROJ_FAINT_BANDS)[band].T
    opac[i] = lo + (hi - lo) * rng.uniform(0.15, 0.85, 40)
    z = rng.uniform(2, 6, 40)
    means[i] = to_world(pix(rng.uniform(4, W - 5, 40), rng.uniform(4, H - 5, 40), z))
    scales[i] = sigma(rng.uniform(2, 9, 40), z)[:, None] * np.exp(0.3 * rng.normal(size=(40, 3)))
    i = take("solid", 24)
    opac[i] = rng.uniform(0.99, 0.9999, 24)
    z = rng.uniform(2, 6, 24)
    means[i] = to_world(pix(rng.uniform(0, W - 1, 24), rng.uniform(0, H - 1, 24), z))
    scales[i] = sigma(rng.uniform(1, 6, 24), z)[:, None] * np.exp(0.3 * rng.normal(size=(24, 3)))
    i = take("needle", 26)
    z = rng.uniform(2, 6, 26)
    means[i] = to_world(pix(rng.uniform(0, W - 1, 26), rng.uniform(0, H - 1, 26), z))
    long_ = sigma(rng.uniform(4, 12, 26), z)     # (longer: the float32 determinant cancels, errors of the ORACLE past 10 x its 99th percentile)
    scales[i] = long_[:, None] / rng.uniform(300, 1000, (26, 3))
    scales[i, rng.randint(0, 3, 26)] = long_
    opac[i] = rng.uniform(0.2, 0.8, 26)
    i = take("speck", 24)
    z = rng.uniform(2, 6, 24)
    means[i] = to_world(pix(rng.uniform(0, W - 1, 24), rng.uniform(0, H - 1, 24), z))
    scales[i] = 1e-4 * z[:, None] * np.ones(3)
    opac[i] = rng.uniform(0.2, 0.8, 24)
    i = take("sheet", 22)
    z = rng.uniform(3, 6, 22)
    means[i] = to_world(pix(rng.uniform(0.3 * W, 0.7 * W, 22), rng.uniform(0.3 * H, 0.7 * H, 22), z))
    scales[i] = sigma(rng.uniform(2.0, 4.0, 22) * max(W, H), z)[:, None] * np.ones(3)
    opac[i] = rng.uniform(0.01, 0.05, 22)
    # quaternions whose length lies either side of F.normalize's eps = 1e-12; four all-zero rows
    i = take("quat", 28)
    v = rng.normal(size=(28, 4))
    rot[i] = v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(math.log(1e-13), math.log(1e-11), 28))[:, None]
    rot[i[:4]] = 0.0
    z = rng.uniform(2, 6, 28)
    means[i] = to_world(pix(rng.uniform(0, W - 1, 28), rng.uniform(0, H - 1, 28), z))
    scales[i] = sigma(rng.uniform(1, 6, 28), z)[:, None] * np.exp(0.5 * rng.normal(size=(28, 3)))
    # near plane, camera B (view = world + (0, 0, 2^-6)): the world z is a float32 and the sum is exact
    i = take("near", 40)
    zv = np.array(PROJ_NEAR_Z)[np.arange(40) % 5]
    zw = (zv - PROJ_CAM_B_TZ).astype(np.float32).astype(np.float64)
    assert ((zw + PROJ_CAM_B_TZ).astype(np.float32).astype(np.float64) == zv).all() and (zw + PROJ_CAM_B_TZ == zv).all()
    means[i] = np.stack([zv * tx * rng.uniform(-0.8, 0.8, 40), zv * ty * rng.uniform(-0.8, 0.8, 40), zw], 1)
    scales[i] = 0.02 * zv[:, None] * np.ones(3)
    opac[i] = rng.uniform(0.2, 0.8, 40)

    perm = (367 * np.arange(P)) % P                       # row j of the scene = row perm[j] of the construction
    inv = np.argsort(perm)
    planted = {k: np.sort(inv[v]) for k, v in planted.items()}
    t32 = lambda a: torch.tensor(np.asarray(a)[perm], dtype=torch.float32)  # noqa: E731
    d.update(means3D=t32(means), scales=t32(scales), opacities=t32(opac).reshape(P, 1), rotations=t32(rot), shs=t32(shs))
    return d, cams, planted


def raw_parameters(d):
    """The raw (pre-activation) parameters a scene dict's activated ones come from: log scales, the quaternion as it is,
    logit opacity, SH rows split into dc / rest -- float32, what the RAW entry points of the library take."""
    op = d["opacities"].double().reshape(-1, 1)
    return dict(xyz=d["means3D"].float().contiguous(), features_dc=d["shs"][:, :1].float().contiguous(),
                features_rest=d["shs"][:, 1:].float().contiguous(), scaling=torch.log(d["scales"].double()).float(),
                rotation=d["rotations"].float().contiguous(), opacity=torch.log(op / (1 - op)).float())


def torch_activations(d):
    """d with scales / rotations / opacities replaced by what the reference's accessors make of raw_parameters(d): exp,
    F.normalize (eps 1e-12), sigmoid in float32 (tests/test_gpu_round5.py pins the kernels' activations to these bits)."""
    raw = raw_parameters(d)
    out = dict(d)
    out.update(scales=torch.exp(raw["scaling"]), rotations=torch.nn.functional.normalize(raw["rotation"]),
               opacities=torch.sigmoid(raw["opacity"]))
    return out


def projection_strata(o, planted, W, H):
    """Boolean masks of PROJ_STRATA for one view from the float64 reference's output `o` (projection_ref.project on the
    activated parameters) -- geometry strata need a visible Gaussian; `planted` only tells needle / speck / sheet / quat /
    solid / faint candidates apart from the crowd, the property itself is checked on the reference's quantities."""
    P = len(o["mx"])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    vis = o["visible"]
    cand = lambda k: np.isin(np.arange(P), planted[k])  # noqa: E731
    m = dict(clamp_x=vis & o["clamp_x"] & ~o["clamp_y"], clamp_y=vis & o["clamp_y"] & ~o["clamp_x"], clamp_xy=vis & o["clamp_x"] & o["clamp_y"])
    zok = o["visible_z"]
    m["edge_l"], m["edge_r"] = zok & (o["mx"] < -0.5), zok & (o["mx"] > W - 0.5)
    m["edge_t"], m["edge_b"] = zok & (o["my"] < -0.5), zok & (o["my"] > H - 0.5)
    rad = o["rad_f"]
    frac = lambda v: np.abs(v - np.round(v))  # noqa: E731
    inside = lambda v, hi: (v > 0.5) & (v < hi + 0.5)  # noqa: E731      (an edge value the clamp does not decide)
    lo, hi_ = (o["mx"] - rad) / 16, (o["mx"] + rad + 15) / 16
    m["align"] = vis & (((frac(lo) < 0.05) & inside(lo, gx)) | ((frac(hi_) < 0.05) & inside(hi_, gx)))
    op = o["opacity"]
    m["faint"] = zok & cand("faint") & (op >= 0.0030) & (op <= 0.006)
    for b, (lo_, hi2) in enumerate(PROJ_FAINT_BANDS):
        m[f"faint{b}"] = m["faint"] & (op >= lo_) & (op < hi2 if b < 3 else op <= hi2) & ((op > lo_) if b == 2 else True)
    m["solid"] = vis & (op >= 0.99)
    m["needle"] = vis & cand("needle")
    m["speck"] = vis & cand("speck") & (np.abs(o["a"] - 0.3) < 1e-3) & (np.abs(o["c"] - 0.3) < 1e-3)
    m["sheet"] = vis & ((o["rect"] == np.array([0, 0, gx, gy])).all(1)) & cand("sheet")
    n = (o["colour_raw"] < 0).sum(1)
    m["ch1"], m["ch2"], m["ch3"] = vis & (n == 1), vis & (n == 2), vis & (n == 3)
    m["quat"] = vis & cand("quat")
    return m


def projection_populations(o, strata, planted, cam, pr):
    """Assert the floors of one view from the float64 reference (non-fragile members: 20 per stratum, 10 for align, 8 per faint
    band, 6 per near value with camera B, 8 per kind of every edge stratum) and the 10 % cap on what a stratum loses to
    fragility -> {stratum: (members, fragile)}"""
    frag = pr.any_fragile(o)
    pop = {}
    for k in PROJ_STRATA + tuple(f"faint{b}" for b in range(4)):
        n, lost = int(strata[k].sum()), int((strata[k] & frag).sum())
        pop[k] = (n, lost)
        floor = 8 if k.startswith("faint") and k != "faint" else PROJ_FLOORS.get(k, 20)
        assert lost <= 0.1 * n, f"camera {cam}: stratum {k} loses {lost} of {n} members to fragility"
        assert n - lost >= floor, f"camera {cam}: stratum {k} holds {n} members, {lost} fragile (floor {floor})"
    for k in ("edge_l", "edge_r", "edge_t", "edge_b"):
        reach, miss = int((strata[k] & o["visible"] & ~frag).sum()), int((strata[k] & ~o["visible"] & ~frag).sum())
        pop[k + " reach/miss"] = (reach, miss)
        assert reach >= 8 and miss >= 8, f"camera {cam}: {k} holds {reach} that reach in and {miss} that do not"
    if cam == "B":
        z = o["pv"][planted["near"], 2]
        counts = [int((z == v).sum()) for v in PROJ_NEAR_Z]
        pop["near"] = counts
        assert min(counts) >= 6 and (o["s_near"][planted["near"]] == 0).all(), f"near values {counts}; view z exact"
        assert (o["visible_z"][planted["near"]] == (z > PROJ_NEAR_Z[0])).all()
    sp = strata["speck"]
    assert (o["radius"][sp] == 3).all(), "a speck is the low-pass filter alone: radius ceil(3 sqrt(0.3 + sqrt(0.1))) = 3"
    ratio = np.sqrt(np.maximum(o["a"], o["c"]) / 0.3)
    assert (strata["needle"].sum() == 0) or np.median(ratio[strata["needle"]]) > 5
    return pop
