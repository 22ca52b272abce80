"""Deterministic cases that sit ON the integer decisions of the splat front end and of the HBM sort — the chunk cull's margins, the near
and far planes, the cheap exclusion, the Jacobian clamp, the conic determinant, depth ties, the deep-tile cull — written once and run
twice, like parity_cases: under the wave64 emulator (test_emu_parity.py) and on the MI355X (test_gpu_parity.py).

parity_cases.check_against_oracle compares these stages bit for bit, but only sees a fault its inputs reach: seeded faults in them passed
every random scene of the suite, or were caught by whichever fuzz seed happened to land on them ("Seeded faults of the front
end").  Every case here therefore
  1. proves FROM THE ORACLE ALONE (oracle_np.preprocess / oracle_c.render and fp64 NumPy), before the library is looked at, that its input
     sits on the decision it is named for;
  2. renders a TWIN moved just across the decision and asserts the opposite outcome for it.
tests/test_emu_frontend_mutants.py seeds the faults and names, per fault, the case and the assertion that must catch it.

A `drv` is a parity_cases driver; chunk_skipped(), set_tuning(morton=...), render_batch() and the debug buffers are used as well.
"""
import dataclasses
import math

import numpy as np

import oracle_c
import oracle_np as onp
import parity_cases as pc
from sage_gs import _capi

EYE = np.eye(4, dtype=np.float32)
SPECK = 1.0e-4                  # a scale far below a pixel at any depth used here: the splat is the dilation's 3-pixel disc


def debug_buffer(drv, what, dtype):
    """A debug buffer of the last frame from either driver (the emulator's reads the C ABI, the GPU's goes through sage_gs.Renderer)."""
    return drv.debug(what, dtype) if hasattr(drv, "debug") else drv.r.debug_buffer(what, dtype)


class caller_order:
    """with caller_order(drv): scenes are uploaded in the caller's order (sgs_tuning.morton = 0), so that 64 consecutive Gaussians ARE a
    chunk — the cases build their chunks by hand and assert the layout from SGS_BUF_SCENE_PERM after the first frame."""

    def __init__(self, drv):
        self.drv = drv

    def __enter__(self):
        self.keep = self.drv.tuning()["morton"]
        self.drv.set_tuning(morton=0)
        return self

    def __exit__(self, *exc):
        self.drv.set_tuning(morton=self.keep)
        return False


def view_to_model(cam, t):
    """View-space points t [n, 3] (fp64) as fp32 model-space means under cam.view (rigid): m = R^T (t - tvec)."""
    V = np.asarray(cam.view, np.float32).astype(np.float64)
    return ((np.asarray(t, np.float64) - V[:3, 3]) @ V[:3, :3]).astype(np.float32)


def at_pixel(cam, px, py, tz):
    """The view-space point that projects to pixel coordinates (px, py) (pixel i has centre coordinate i) at depth tz."""
    return np.array([(px - cam.cx + 0.5) * tz / cam.fx, (py - cam.cy + 0.5) * tz / cam.fy, tz], np.float64)


def make_scene(means, scales, quats=None, opac=0.8, seed=0):
    n = len(means)
    rng = np.random.default_rng(seed)
    q = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)) if quats is None else np.asarray(quats, np.float32)
    o = np.full(n, opac, np.float32) if np.isscalar(opac) else np.asarray(opac, np.float32)
    sh = rng.uniform(-1.0, 1.5, (n, 1, 3)).astype(np.float32)
    return np.ascontiguousarray(means, np.float32), np.ascontiguousarray(scales, np.float32), q, o, sh, 0


# ------------------------------------------------------------------------------------------------------------------------------------------
# Chunk cull margins (sgs_kernels.h chunk_outside, k_chunk_cull, k_chunk_cull_group)
#
# A chunk is kept if its bounding sphere (c, R) of means, padded, can reach the frame: for the near / far planes  tz_c + R' >= near,
# tz_c - R' <= far;  for each side plane (through the camera centre, unit inward normal n, moved outward by c0 pixels)
# n . c + R' + A s_max / |n| >= 0,  with A s_max the allowance for the largest scale of the chunk.  Both margins were cut by seeded faults
# (R' = 0.9 R; half the allowance) without any test noticing.  Two kinds of chunk, built by hand in VIEW space and carried into model space:
#   'R'  sixty-four specks on a segment of length 2 R along a plane's normal: one MEMBER at the inner end, one at the outer end, the rest at the
#        midpoint, which is the sphere's centre (the box's centre of collinear points).  The member's mean lies one pixel OUTSIDE the
#        frame (or 0.03 / 0.05 inside the near / far plane) and reaches it through its 3-sigma disc; the sphere crosses the plane by less than
#        R / 20, so a radius of 0.95 R loses the member;
#   'S'  sixty-four Gaussians at ONE point (R = 0) far outside the frame beyond both Jacobian clamps, one of them — the member — so large
#        that its 3-sigma square reaches the frame by four pixels: only the scale allowance keeps the chunk, and more than half of it is used.
MARGIN_RES = (200, 150)
MARGIN_FAR = 10.0
BAND = (3, 6)                   # the band of tile rows of the band-edge chunks (frame: 10 rows)
SIDE_R, SIDE_TZ = 2.0, 2.0      # radius of the side-plane chunks and depth of their members
TWIN_SHIFT = 0.05               # the twin's chunks lie this share of their radius further out ('S' chunks: see margin_chunks)


def margin_cameras():
    """The identity view; a yawed, pitched and rolled one; one with the principal point off centre and fx != fy."""
    w, h = MARGIN_RES
    return {"identity": onp.Camera(w, h, 150.0, 150.0, w / 2.0, h / 2.0, EYE.copy()),
            "turned": onp.Camera(w, h, 150.0, 150.0, w / 2.0, h / 2.0, pc.look_at_view((0.4, -0.3, -0.5), (1.5, 0.6, 4.0), down=(0.1, 1.0, 0.05))),
            "off_centre": onp.Camera(w, h, 170.0, 120.0, 83.3, 91.7, EYE.copy())}


def _side_plane(cam, side, edge):
    """Unit inward normal (view space) of the plane through the camera centre and the pixel line px = edge (left / right) or py = edge."""
    n = {"left": (cam.fx, 0.0, cam.cx - 0.5 - edge), "right": (-cam.fx, 0.0, edge - cam.cx + 0.5),
         "top": (0.0, cam.fy, cam.cy - 0.5 - edge), "bottom": (0.0, -cam.fy, edge - cam.cy + 0.5)}[side]
    n = np.array(n, np.float64)
    return n / np.linalg.norm(n)


def margin_chunks(cam, cfg, twin=False):
    """The hand-made chunks of one camera: (scene, list of chunk records).  A record: name, kind, member (index into the scene), centre and
    radius in view space, the plane's inward normal (None for 'S'), when the chunk is looked at ('frame', 'band')."""
    w, h = cam.width, cam.height
    gx, gy = cam.grid
    recs, means, scales, quats = [], [], [], []

    def add_segment(name, member, n, R, when):
        """kind 'R': member at `member`, the sphere's centre R behind it along -n."""
        shift = TWIN_SHIFT * R if twin else 0.0
        inner = member - shift * n
        pts = np.repeat((inner - R * n)[None], 64, 0)
        lane = (7 * len(recs) + 3) % 64
        pts[lane] = inner; pts[(lane + 31) % 64] = inner - 2.0 * R * n
        recs.append(dict(name=name, kind="R", member=64 * len(recs) + lane, centre=inner - R * n, R=R, n=n, when=when))
        means.append(pts); scales.append(np.full((64, 3), SPECK)); quats.append(np.tile([1.0, 0, 0, 0], (64, 1)))

    # the four side planes of the frame, and both edges of the band of tile rows: the member 1 px outside (the right / bottom edges are the
    # tile grid's: S3 clips rects to tiles, and a tile holds 16 pixels whether the frame has them or not)
    edges = dict(left=-0.5, right=16 * gx - 0.5, top=-0.5, bottom=16 * gy - 0.5)
    mid_x, mid_y = 0.37 * w, 0.5 * (16 * BAND[0] + 16 * BAND[1])
    for side in ("left", "right", "top", "bottom"):
        out = -1.0 if side in ("left", "top") else 1.0
        p = (edges[side] + out * 1.0, mid_y) if side in ("left", "right") else (mid_x, edges[side] + out * 1.0)
        add_segment(side, at_pixel(cam, p[0], p[1], SIDE_TZ), _side_plane(cam, side, edges[side]), SIDE_R, "frame")
    for side, edge in (("top", 16 * BAND[0] - 0.5), ("bottom", 16 * BAND[1] - 0.5)):
        out = -1.0 if side == "top" else 1.0
        add_segment("band_" + side, at_pixel(cam, 0.61 * w, edge + out * 1.0, SIDE_TZ), _side_plane(cam, side, edge), SIDE_R, "band")
    # near and far: the member 0.03 / 0.05 inside the plane
    add_segment("near", at_pixel(cam, 0.3 * w, mid_y, cfg.near + 0.03), np.array([0.0, 0.0, 1.0]), 1.0, "frame")
    add_segment("far", at_pixel(cam, 0.7 * w, mid_y, cfg.far - 0.05), np.array([0.0, 0.0, -1.0]), 2.0, "frame")
    # kind 'S': at the frame's corners beyond both clamps (|tx / tz| > limx, |ty / tz| > limy: the projected size is largest there); the
    # second one a NEEDLE whose long axis is the direction the clamped Jacobian stretches most — it points at the image
    limx, limy = cfg.clamp * 0.5 * w / cam.fx, cfg.clamp * 0.5 * h / cam.fy
    tz = 4.0
    for name, sx, needle in (("scale_left", -1.0, False), ("scale_right", 1.0, True)):
        s_big = 160.0 * tz / max(cam.fx, cam.fy)
        J = np.array([[cam.fx / tz, 0.0, -cam.fx * sx * limx / tz], [0.0, cam.fy / tz, cam.fy * limy / tz]])        # clamped: (sx limx, -limy)
        _, sv, vt = np.linalg.svd(J)
        lam = (sv[0] * s_big) ** 2 + cfg.dilation
        reach = math.ceil(3.0 * math.sqrt(lam)) - 4.0                        # (the isotropic member's radius is a little larger: checked by the oracle)
        A_px = 1.001 * 3.0 * math.sqrt(2.0 * (2.0 + limx * limx + limy * limy)) * max(cam.fx, cam.fy) * s_big / tz     # the allowance in pixels
        px = (-0.5 - reach) if sx < 0 else (16 * gx - 0.5 + reach)
        if twin:                # beyond the whole allowance and the constant slack (c0 < 8 px), 0.1 % for the comparison's own slack
            px = (-0.5 - 1.001 * (A_px + 8.0)) if sx < 0 else (16 * gx - 0.5 + 1.001 * (A_px + 8.0))
        py = cam.cy - 0.5 - 1.2 * limy * cam.fy
        assert abs((px - cam.cx + 0.5) / cam.fx) > 1.05 * limx
        c = at_pixel(cam, px, py, tz)
        lane = (7 * len(recs) + 3) % 64
        sc = np.full((64, 3), SPECK); q = np.tile([1.0, 0, 0, 0], (64, 1))
        if needle:              # model-space long axis = R^T (the right singular vector of J's largest singular value)
            V = np.asarray(cam.view, np.float32).astype(np.float64)
            axis = V[:3, :3].T @ (vt[0] if (V[:3, :3].T @ vt[0])[0] >= 0.0 else -vt[0])
            sc[lane] = (s_big, 1.0e-3, 1.0e-3)
            cr = np.cross([1.0, 0.0, 0.0], axis)
            q[lane] = np.array([1.0 + axis[0], *cr]) / np.linalg.norm([1.0 + axis[0], *cr])
        else:
            sc[lane] = s_big
        recs.append(dict(name=name, kind="S", member=64 * len(recs) + lane, centre=c, R=0.0, n=None, when="frame",
                         reach=reach, A_px=A_px, edge_dist=abs(px - (-0.5 if sx < 0 else 16 * gx - 0.5))))
        means.append(np.repeat(c[None], 64, 0)); scales.append(sc); quats.append(q)
    scene = make_scene(view_to_model(cam, np.concatenate(means)), np.concatenate(scales), np.concatenate(quats), seed=3)
    return scene, recs


def _chunk_skipped_after(drv, render):
    render()
    return np.asarray(drv.chunk_skipped()).astype(bool)


def case_chunk_margins(drv, which="identity"):
    """The chunk cull's two margins, the sphere's padding and the scale allowance, on each of the four side planes, the near plane, the far
    plane and both edges of a band of tile rows (contiguous, and interleaved with stride 2), for one of margin_cameras(); through
    k_chunk_cull (one frame) and k_chunk_cull_group (a batch of three).
    From the oracle alone: every member is visible (and in a band: in that band), nothing else is, every sphere's centre is outside its plane
    by more than 0.95 R ('R' chunks) or by more than the constant slack plus half the scale allowance ('S' chunks, R = 0).
    The library: SGS_BUF_CHUNK_SKIPPED says 'kept' for every one of these chunks, the frame is the oracle's (check_against_oracle).
    The twin (every chunk 0.05 R further out; 'S' chunks beyond the allowance): the oracle sees nothing, SGS_BUF_CHUNK_SKIPPED says 'skipped'."""
    cam = margin_cameras()[which]
    cfg = onp.Config(far=MARGIN_FAR)
    c0 = 1.001 * (3.0 * math.sqrt(2.0 * cfg.dilation + 0.3163) + 1.0) + 0.5 + 1.0       # the constant slack of a side plane, in pixels
    with caller_order(drv):
        for twin in (False, True):
            scene, recs = margin_chunks(cam, cfg, twin)
            tag = f"chunk margins [{which}{', twin' if twin else ''}]"
            members = np.array([r["member"] for r in recs])
            # ---- the oracle alone
            pre = onp.preprocess(*scene, cam, cfg)
            pre_band = onp.preprocess(*scene, cam, cfg, BAND[0], BAND[1])
            if not twin:
                assert sorted(np.nonzero(pre["visible"])[0]) == sorted(members), f"{tag}: the oracle sees {np.nonzero(pre['visible'])[0]}, the members are {members}"
                assert pre_band["visible"][[r["member"] for r in recs if r["when"] == "band"]].all(), f"{tag}: a band-edge member is not in the band"
                xy = pre["xy64"]
                for r in recs:
                    x, y = xy[r["member"]]
                    inside = -0.5 <= x <= cam.width - 0.5 and -0.5 <= y <= cam.height - 0.5
                    assert r["when"] == "band" or r["name"] in ("near", "far") or not inside, f"{tag}: {r['name']}: the member's mean is inside the frame"
                    if r["kind"] == "R" and r["name"] not in ("near", "far"):
                        d = -float(r["n"] @ r["centre"])
                        assert 0.95 * r["R"] < d <= r["R"] * (1.0 + 1e-9) + 2.0 * SIDE_TZ / min(cam.fx, cam.fy), (tag, r["name"], d)
                    if r["kind"] == "S":
                        assert r["edge_dist"] > c0 + 2.0 + 0.505 * r["A_px"] and r["edge_dist"] < pre["radius"][r["member"]], (tag, r["name"], r["edge_dist"], r["A_px"])
                near, far = next(r for r in recs if r["name"] == "near"), next(r for r in recs if r["name"] == "far")
                assert near["centre"][2] + 0.95 * near["R"] < cfg.near < near["centre"][2] + near["R"]
                assert far["centre"][2] - 0.95 * far["R"] > cfg.far > far["centre"][2] - far["R"]
            else:
                band_m = [r["member"] for r in recs if r["when"] == "band"]          # (moved out of the band, still inside the frame)
                assert sorted(np.nonzero(pre["visible"])[0]) == sorted(band_m) and not pre_band["visible"].any(), f"{tag}: the oracle sees {np.nonzero(pre['visible'])[0]}"
            # ---- the library
            drv.upload(*scene)
            looks = [("frame", lambda: drv.render(cam, cfg), [r for r in recs if r["when"] == "frame"]),
                     ("band", lambda: drv.render(cam, cfg, BAND), [r for r in recs if r["when"] == "band"]),
                     ("batch", lambda: drv.render_batch([margin_cameras()["off_centre" if which != "off_centre" else "turned"], cam, cam], cfg=cfg),
                      [r for r in recs if r["when"] == "frame"])]
            # interleaved rows span the frame: its top and bottom planes are the frame's, whichever rows the call owns
            for phase in (0, 1):
                looks.append((f"interleave (2, {phase})", lambda phase=phase: drv.render(cam, cfg, interleave=(2, phase)),
                              [r for r in recs if r["name"] in ("top", "bottom")]))
            for what, render, rs in looks:
                sk = _chunk_skipped_after(drv, render)
                if what == "frame":
                    assert (debug_buffer(drv, _capi.BUF_SCENE_PERM, np.uint32) == np.arange(len(scene[0]))).all(), f"{tag}: the layout is not the caller's order"
                    assert len(sk) == len(recs)
                for r in rs:
                    k = r["member"] // 64
                    if twin:
                        assert sk[k], f"{tag}: {what}: chunk '{r['name']}' is KEPT although no Gaussian inside its bounds can reach the frame"
                    else:
                        assert not sk[k], f"{tag}: {what}: chunk '{r['name']}' is SKIPPED although its member {r['member']} is visible"
            for rows, ref in (((0, -1), pre), (BAND, pre_band)):          # the per-Gaussian decisions: the members are specks AT the edges
                drv.render(cam, cfg, rows, full_sort=True, loose_cull=True)
                got, exp = sorted(int(i) for i in drv.intermediates()[2]), [int(i) for i in np.nonzero(ref["visible"])[0]]
                assert got == exp, f"{tag}: rows {rows}: the library sees the Gaussians {got}, the oracle {exp}"
            if not twin:
                img, st, aux, _ = pc.check_against_oracle(drv, scene, cam, cfg, what=tag)
                assert st["n_visible"] == len(recs)
                pc.check_against_oracle(drv, scene, cam, cfg, rows=BAND, what=tag + " band", thorough=False)


# ------------------------------------------------------------------------------------------------------------------------------------------
# Near and far planes: tz > near, tz <= far (preprocess_chunk's `front`)
def ulp_neighbours(v):
    v = np.float32(v)
    return np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))


def case_near_far_equality(drv):
    """Six specks under the identity view (tz is the stored z, exactly), at distinct pixels: z one fp32 ulp below near_z, equal to it, one ulp
    above; the same around far_z.  near_z and far_z are exact in fp32 (0.25 and 8), so the oracle's fp64 constants are the library's.
    From the oracle alone: visible are exactly z = near + ulp, far - ulp and far (tz > near, tz <= far) — each visible speck has its twin one
    ulp away on the other side.  The library must see the same three (the known-answer cases only ever had z = 10.5 against far = 10)."""
    cam = onp.Camera(96, 64, 80.0, 80.0, 48.0, 32.0, EYE.copy())
    cfg = onp.Config(near=0.25, far=8.0)
    zs = np.array(ulp_neighbours(cfg.near) + ulp_neighbours(cfg.far), np.float32)
    assert len(set(zs.tolist())) == 6 and zs[1] == cfg.near and zs[4] == cfg.far
    means = np.stack([at_pixel(cam, 10.0 + 15.0 * i, 20.0 + 4.0 * i, 1.0) * float(z) for i, z in enumerate(zs)]).astype(np.float32)
    means[:, 2] = zs
    scene = make_scene(means, np.full((6, 3), SPECK), seed=5)
    want = [2, 3, 4]
    pre = onp.preprocess(*scene, cam, cfg)
    assert list(np.nonzero(pre["visible"])[0]) == want, f"near / far equality: the oracle sees {np.nonzero(pre['visible'])[0]}"
    drv.upload(*scene)
    _, st = drv.render(cam, cfg, full_sort=True, loose_cull=True)           # (the test hooks' render: intermediates() reads its queues)
    got = sorted(int(i) for i in drv.intermediates()[2])
    names = ["near - ulp", "near", "near + ulp", "far - ulp", "far", "far + ulp"]
    assert got == want and st["n_visible"] == 3, \
        f"near / far equality: the library sees z = {[names[i] for i in got]}, the oracle {[names[i] for i in want]} (tz > near_z, tz <= far_z)"
    pc.check_against_oracle(drv, scene, cam, cfg, what="near / far equality")


# ------------------------------------------------------------------------------------------------------------------------------------------
# Cheap exclusion and Jacobian clamp (preprocess_chunk): giants beyond both clamps whose S3 rect reaches the frame by less than a pixel
GIANT_X = 60.0                  # f s / tz of the giants, in pixels (their 3-sigma radius is ~4.4 times that beyond both clamps)


def clamped_giants(cam, cfg, twin=False):
    """One isotropic giant per side of the frame and per edge of the band BAND, each beyond BOTH clamps (|tx / tz| > limx and |ty / tz| > limy)
    with the edge of its S3 square 0.75 px inside the first pixel column / row that makes its tile rect non-empty (twin: 0.75 px outside).
    Returns (scene, names)."""
    w, h = cam.width, cam.height
    gx, gy = cam.grid
    limx, limy = cfg.clamp * 0.5 * w / cam.fx, cfg.clamp * 0.5 * h / cam.fy
    tz = 5.0
    s = GIANT_X * tz / max(cam.fx, cam.fy)
    off_x, off_y = cam.cx - 0.5 + 1.25 * limx * cam.fx, cam.cy - 0.5 - 1.25 * limy * cam.fy      # beyond the clamp of the OTHER axis
    # the radius beyond both clamps does not depend on where: take it from the oracle at a provisional place
    probe = make_scene(view_to_model(cam, [at_pixel(cam, -3.0 * w, off_y, tz)]), np.full((1, 3), s))
    rad = float(onp.preprocess(*probe, cam, cfg)["radius"][0])
    d = -0.75 if twin else 0.75
    spots = {"left": (1.0 - rad + d, off_y), "right": (16 * gx + rad - d, off_y), "top": (off_x, 1.0 - rad + d), "bottom": (off_x, 16 * gy + rad - d),
             "band_first_row": (off_x, 16 * BAND[0] + 1.0 - rad + d), "band_last_row": (off_x, 16 * BAND[1] + rad - d)}
    # (right / bottom: the rect is non-empty while floor((p - rad) / 16) < grid, i.e. p - rad < 16 grid: the twin sits ON or beyond it)
    means = np.array([at_pixel(cam, px, py, tz) for px, py in spots.values()])
    return make_scene(view_to_model(cam, means), np.full((len(spots), 3), s), opac=0.3, seed=7), list(spots), rad


def case_clamped_giants(drv, which="identity"):
    """The cheap fp32 exclusion's bound and the Jacobian clamp, where both matter most: a Gaussian beyond both clamps is the one whose exact
    radius, 3 sqrt(lambda_max) with lambda_max = (f s / tz)^2 (1 + limx^2 + limy^2) (+ dilation), comes closest to the bound rb that the
    exclusion derives from (f s / tz)^2 (2 + limx^2 + limy^2) — rb / radius = sqrt(2 (2 + l^2) / (1 + l^2)) there, 1.7 at the default clamp;
    nothing comes closer, rb is never within per cents of the radius.
    From the oracle alone: every giant is visible with a rect one tile wide (or high) at its edge; |tx / tz| > limx and |ty / tz| > limy for each and
    the radius WITHOUT the clamp (cfg.clamp = 1e6) is larger: the clamp is active.  The twin, 1.5 px further out, is invisible (band giants: in
    the band).  The library: the same visible sets, the oracle's rects bit for bit (check_against_oracle)."""
    cam = margin_cameras()[which]
    cfg = onp.Config()
    limx, limy = cfg.clamp * 0.5 * cam.width / cam.fx, cfg.clamp * 0.5 * cam.height / cam.fy
    for twin in (False, True):
        scene, names, rad = clamped_giants(cam, cfg, twin)
        tag = f"clamped giants [{which}{', twin' if twin else ''}]"
        n = len(names)
        band_ids = [i for i, nm in enumerate(names) if nm.startswith("band")]
        pre, pre_band = onp.preprocess(*scene, cam, cfg), onp.preprocess(*scene, cam, cfg, BAND[0], BAND[1])
        loose = onp.preprocess(*scene, cam, dataclasses.replace(cfg, clamp=1.0e6))
        V = np.asarray(cam.view, np.float32).astype(np.float64)
        t = scene[0].astype(np.float64) @ V[:3, :3].T + V[:3, 3]
        assert (np.abs(t[:, 0] / t[:, 2]) > limx).all() and (np.abs(t[:, 1] / t[:, 2]) > limy).all() and (loose["radius"] > pre["radius"]).all(), f"{tag}: a clamp is not active"
        assert (pre["radius"] == rad).all()
        want = [] if twin else list(range(n))
        want_frame = band_ids if twin else want               # (the twins of the band's giants have left the band, not the frame)
        assert list(np.nonzero(pre["visible"])[0]) == want_frame and [i for i in np.nonzero(pre_band["visible"])[0] if i in band_ids] == (band_ids if not twin else []), \
            f"{tag}: the oracle sees {np.nonzero(pre['visible'])[0]} / in the band {np.nonzero(pre_band['visible'])[0]}"
        if not twin:
            r = pre["rect"]
            assert (np.minimum(r[:4, 2] - r[:4, 0], r[:4, 3] - r[:4, 1]) == 1).all(), f"{tag}: a giant reaches more than one tile deep into the frame: {r}"
        drv.upload(*scene)
        for rows, ids, ref in (((0, -1), list(range(n)), pre), (BAND, band_ids, pre_band)):
            _, st = drv.render(cam, cfg, rows, full_sort=True, loose_cull=True)
            _, _, slot_ids, splats = drv.intermediates()
            got = sorted(int(i) for i in slot_ids if int(i) in ids)
            exp = [i for i in ids if ref["visible"][i]]
            assert got == exp, f"{tag}: rows {rows}: the library sees {[names[i] for i in got]}, the oracle {[names[i] for i in exp]}"
            for i, sp in zip(slot_ids, splats):
                rect = (int(sp[10]) & 0xffff, int(sp[10]) >> 16, int(sp[11]) & 0xffff, int(sp[11]) >> 16)
                want_rect = tuple(int(v) for v in ref["rect"][i])
                assert rect == want_rect, f"{tag}: rows {rows}: the tile rect of giant '{names[i]}' is {rect}, the oracle's {want_rect}"
        pc.check_against_oracle(drv, scene, cam, cfg, what=tag, thorough=not twin)
        pc.check_against_oracle(drv, scene, cam, cfg, rows=BAND, what=tag + " band", thorough=False)


# ------------------------------------------------------------------------------------------------------------------------------------------
# Determinant precision: det = a c - b^2 of a needle's 2-D covariance
def case_needle_determinant(drv):
    """Needles of aspect 2000 (sigma_major 1500 px, sigma_minor the dilation's 0.55 px) through the frame at five angles: a c and b^2 agree to
    six digits, and det = a c - b^2 formed in fp32 is off by per cents — stated here from fp64 NumPy: every needle loses more than 1e-5
    relative (the conic's tolerance in check_against_oracle), so a determinant evaluated in fp32 fails the conic check on every one.
    (No twin: det > 0 holds for every finite Gaussian under a positive dilation; there is no other side to move to.)"""
    cam = onp.Camera(128, 96, 150.0, 150.0, 64.0, 48.0, EYE.copy())
    cfg = onp.Config()
    tz, n = 5.0, 5
    s_long = 1500.0 * tz / cam.fx
    ang = np.deg2rad([15.0, 30.0, 45.0, 60.0, 75.0])
    quats = np.stack([np.cos(ang / 2), np.zeros(n), np.zeros(n), np.sin(ang / 2)], 1)            # about the view axis
    means = np.stack([at_pixel(cam, 20.0 + 22.0 * i, 30.0 + 9.0 * i, tz) for i in range(n)]).astype(np.float32)
    scales = np.tile(np.array([s_long, s_long / 2000.0, s_long / 2000.0]), (n, 1))
    scene = make_scene(means, scales, quats, opac=0.4, seed=9)
    pre = onp.preprocess(*scene, cam, cfg)
    assert pre["visible"].all()
    c64 = pre["conic64"]                              # (c, -b, a) / det
    det = 1.0 / (c64[:, 0] * c64[:, 2] - c64[:, 1] ** 2)
    a, b, c = c64[:, 2] * det, -c64[:, 1] * det, c64[:, 0] * det
    a32, b32, c32 = (v.astype(np.float32) for v in (a, b, c))
    det32 = (a32 * c32 - b32 * b32).astype(np.float64)
    loss = np.abs(det32 - det) / det
    assert (loss > 1.0e-5).all() and (np.sqrt(a + c) / np.sqrt(det / (a + c)) >= 1.0e3).all(), f"needle determinant: fp32 loses only {loss} on aspects {np.sqrt(a + c) / np.sqrt(det / (a + c))}"
    drv.upload(*scene)
    drv.render(cam, cfg, full_sort=True, loose_cull=True)
    _, _, slot_ids, splats = drv.intermediates()
    assert sorted(slot_ids) == list(range(n)), f"needle determinant: the library sees {sorted(slot_ids)}"
    f = splats[np.argsort(slot_ids)].view(np.float32)
    rel = np.abs(f[:, 2:5] - pre["conic"]) / np.maximum(np.abs(pre["conic"]), 1e-6 * np.abs(pre["conic"]).max(axis=1, keepdims=True))
    assert rel.max() < 1.0e-5, f"needle determinant: the library's conic is off by {rel.max():.2e} relative (fp32 would lose {loss.min():.1e} .. {loss.max():.1e})"
    pc.check_against_oracle(drv, scene, cam, cfg, what="needle determinant", thorough=False)


# ------------------------------------------------------------------------------------------------------------------------------------------
# Depth ties in the HBM sort (sort_segment): short runs fixed in place
TIE_RUNS = (2, 3, 31, 32, 33, 2, 3)          # lengths of the runs of equal depth bits; SGS_TIE_RUN_MAX is 32, so 33 takes the (index, depth) resort


def tie_run_scene(runs=TIE_RUNS, resort=True):
    """One 16x16-pixel tile covered by every splat.  Depth bits, as offsets from those of z = 1:
      a CLUSTER of 1100-odd records on consecutive bit patterns from 5 * 2^19 + 4096 on, with runs of `runs` equal patterns inside it — the
      first run on the cluster's lowest pattern, the last on its highest;
      one OUTLIER 300 000 patterns above the cluster; 300 records spread up to z = 1000.
    The queue spans ten octaves, so its 256 depth buckets are 2^19 patterns wide and cluster and outlier share one; refined over ITS range
    (300 000 patterns: sub-buckets of 2^11) the cluster stays in ONE sub-bucket of more than SGS_QCAP = 1024 records: radix-sorted through
    HBM, its tie runs fixed in place.  resort=False: without the run of 33.
    Inside a run the x coordinate DEcreases with the index (y and z equal), so the Z-order layout holds a run in descending index order:
    the records reach the sort's fix-up last-index-first.  Returns (scene, camera, [index arrays of the runs])."""
    runs = tuple(r for r in runs if resort or r <= 32)
    base = np.float32(1.0).view(np.uint32) + np.uint32(5 * (1 << 19) + 4096)
    n_distinct = 1100
    at = np.linspace(0, n_distinct - 1, len(runs)).astype(int)           # which distinct patterns carry the runs: the first, ..., the last
    mult = np.ones(n_distinct, int); mult[at] = runs
    bits = np.repeat(base + np.arange(n_distinct, dtype=np.uint32), mult)
    run_of = np.repeat(np.where(mult > 1, np.arange(n_distinct), -1), mult)
    rng = np.random.default_rng(11)
    n_c = len(bits)
    z_c = bits.view(np.float32)
    z_out = np.array([base + np.uint32(n_distinct + 300_000)], np.uint32).view(np.float32)
    z_rest = np.exp(rng.uniform(0.0, math.log(1000.0), 300)).astype(np.float32); z_rest[0], z_rest[1] = 1.0, 1000.0
    z = np.concatenate([z_c, z_out, z_rest])
    n = len(z)
    x = rng.uniform(-0.1, 0.1, n); y = rng.uniform(-0.1, 0.1, n)
    order = rng.permutation(n)                       # the cluster is scattered over the scene's indices
    inv = np.empty(n, int); inv[order] = np.arange(n)
    run_ids = []
    for r in np.unique(run_of[run_of >= 0]):
        idx = np.sort(inv[np.nonzero(run_of == r)[0]])               # the run's indices in the final scene, ascending
        run_ids.append(idx)
    means = np.stack([x, y, z], 1).astype(np.float32)[order]
    for idx in run_ids:                                             # x decreases with the index, y equal
        means[idx, 0] = np.linspace(0.09, -0.09, len(idx)).astype(np.float32); means[idx, 1] = means[idx[0], 1]
    scales = (2.0 * means[:, 2:3] * np.ones((1, 3))).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    opac = rng.uniform(0.005, 0.012, n).astype(np.float32)
    scene = (means, scales, quats, opac, rng.normal(size=(n, 1, 3)).astype(np.float32), 0)
    return scene, onp.Camera(16, 16, 16.0, 16.0, 8.0, 8.0, EYE.copy()), run_ids


def case_short_tie_runs(drv, resort=False):
    """Runs of 2, 3, 31 and 32 equal depth bits (resort=True: and 33, which sends the segment through the (index, depth) resort instead) inside a
    depth bucket that is sorted through HBM (tie_run_scene).  From the oracle alone: the runs are runs — equal depth bits, queue positions
    adjacent, ascending index; the first run opens the cluster, the last closes it.  From SGS_BUF_SCENE_PERM: inside every run the layout
    order is the REVERSE of the index order.  The library: one bucket sorted through HBM (n_spill_tiles), the oracle's queue bit for bit.
    (The twin of a tie is the same record one bit pattern away: the cluster's thousand singletons.)"""
    scene, cam, run_ids = tie_run_scene(resort=resort)
    tag = f"short tie runs [{'with' if resort else 'without'} a run of 33]"
    _, aux = oracle_c.render(*scene, cam)
    ids, bits = aux["ids"], aux["depth_bits"]
    assert aux["n_visible"] == len(scene[0]) == aux["D"]
    pos = np.empty(len(ids), int); pos[ids] = np.arange(len(ids))
    cluster = np.nonzero((bits >= bits[run_ids[0][0]]) & (bits <= bits[run_ids[-1][0]]))[0]
    for idx in run_ids:
        assert (bits[idx] == bits[idx[0]]).all() and (np.diff(pos[idx]) == 1).all(), f"{tag}: {idx} is not a run of the oracle's queue"
    assert pos[run_ids[0][0]] == pos[cluster].min() and pos[run_ids[-1][-1]] == pos[cluster].max() and len(cluster) > 1024
    assert sorted(len(i) for i in run_ids) == sorted(r for r in TIE_RUNS if resort or r <= 32)
    drv.upload(*scene)
    img, st = drv.render(cam, fine=False)
    perm = debug_buffer(drv, _capi.BUF_SCENE_PERM, np.uint32).astype(np.int64)          # layout position -> original index
    where = np.empty(len(perm), int); where[perm] = np.arange(len(perm))
    for idx in run_ids:
        assert (np.diff(where[idx]) < 0).all(), f"{tag}: run {idx}: the layout order is not the reverse of the index order"
    assert st["n_spill_tiles"] >= 1, f"{tag}: no depth bucket was sorted through HBM"
    _, st_full = drv.render(cam, full_sort=True, fine=False)
    got = drv.intermediates()[1]
    bad = np.nonzero(got != ids)[0]
    assert len(bad) == 0, (f"{tag}: the queue differs from (depth bits, index) order at {len(bad)} positions, first at {bad[0]}: "
                           f"index {got[bad[0]]} (bits {bits[got[bad[0]]]:#x}) where the oracle has {ids[bad[0]]} (bits {bits[ids[bad[0]]]:#x})")
    pc.check_against_oracle(drv, scene, cam, what=tag, thorough=False)


# ------------------------------------------------------------------------------------------------------------------------------------------
def case_batch_groups_of_eight(drv, n=1500, res=(96, 64)):
    """A batch whose launch groups hold EIGHT full frames each (sixteen cameras: sgs_render_batch deals them to sgs_tuning.group_lanes = 2 streams,
    eight to a group, sgs_tuning.group's default and SGS_MAX_GROUP): every bit of the frame field of k_chunk_cull_group's work-list entries
    (chunk << 3 | frame) is used, by sixteen DISTINCT views (the 260-frame batches of case_status_ring fill groups of eight with the same
    four cameras of a four-tile frame).  Views a sixteenth of a turn apart inside a cloud: each frame wants other chunks.  Every frame of the batch is the frame rendered alone, bit for bit."""
    scene = pc.random_scene(n, 78, 1, box=((-4, 4), (-2, 2), (-4, 4)), scale=(0.03, 0.25))
    drv.upload(*scene)
    t = drv.tuning()
    assert (t["group"], t["group_lanes"]) == (8, 2), t
    w, h = res
    cams = []
    for k in range(16):
        a = np.deg2rad(22.5 * k + 10.0)
        eye = (0.2, 0.1, -0.1)
        cams.append(onp.Camera(w, h, 0.7 * w, 0.7 * w, w / 2.0, h / 2.0, pc.look_at_view(eye, (eye[0] + np.sin(a), eye[1], eye[2] + np.cos(a)))))
    alone = [drv.render(c, stats=False) for c in cams]
    assert len({st["n_tiles"] for _, st in alone}) == 1, "the frames choose different tilings: a group ends where the tiling changes"
    alone = [a for a, _ in alone]
    assert all(a.max() > 0.05 for a in alone) and all((alone[i] != alone[j]).any() for i in range(16) for j in range(i))
    batch = drv.render_batch(cams)
    for i, a in enumerate(alone):
        assert (batch[i] == a).all(), f"batch groups of eight: frame {i} differs from the frame rendered alone"


# ------------------------------------------------------------------------------------------------------------------------------------------
# Deep-tile cull (k_tile_render): the ends of a culled window
HOLE = (slice(3, 8), slice(8, 13))            # rows 3..7, columns 8..12 of a tile: the 25 pixels no front splat covers


def deep_window_scene(survivor, twin=False, n_back=300):
    """One 16x16-pixel tile.  FRONT: three layers (z = 1, 1.05, 1.1) of opaque specks, one per pixel outside HOLE — three batches, after which
    only the hole's 25 pixels are live and the tile turns to the deep-tile cull: the rest of its queue, resident in LDS, is ONE window.
    BACK: n_back specks between z = 3 and 40 on pixels at least four away from the hole (no pixel they reach is live), and the SURVIVOR, a
    splat over the hole — 'last': at z = 100, behind everything, alone in the queue's last depth bucket: the window's last record;
    'first': at z = 2, in front of the rest of the back, alone in its bucket: the window's first record.
    twin: the survivor sits over the tile's far corner instead and reaches no live pixel — the window has NO survivor.
    Returns (scene, camera, the survivor's index)."""
    rng = np.random.default_rng(41 if survivor == "last" else 42)
    f, c = 16.0, 8.0
    ys, xs = np.mgrid[0:16, 0:16]
    hole = np.zeros((16, 16), bool); hole[HOLE] = True
    px, py = xs[~hole].astype(np.float64), ys[~hole].astype(np.float64)
    front = [np.stack([(px - c + 0.5) * z / f, (py - c + 0.5) * z / f, np.full(px.shape, z)], 1) for z in (1.0, 1.05, 1.1)]
    far = (xs <= 3) | (ys >= 12)                                           # >= 4 pixels from the hole
    k = rng.integers(0, int(far.sum()), n_back)
    zb = np.sort(rng.uniform(3.0, 40.0, n_back))
    back = np.stack([(xs[far][k] - c + 0.5) * zb / f, (ys[far][k] - c + 0.5) * zb / f, zb], 1)
    zs = 100.0 if survivor == "last" else 2.0
    at = (1.0, 14.0) if twin else (10.0, 5.0)                              # pixel (x, y): the far corner / the hole's centre
    surv = np.array([[(at[0] - c + 0.5) * zs / f, (at[1] - c + 0.5) * zs / f, zs]])
    means = np.concatenate(front + [back, surv]).astype(np.float32)
    nf = 3 * len(px)
    scales = np.concatenate([np.repeat((0.55 * means[:nf, 2] / f)[:, None], 3, 1), np.repeat((0.6 * zb / f)[:, None], 3, 1),
                             np.full((1, 3), 1.2 * zs / f)]).astype(np.float32)
    opac = np.concatenate([np.full(nf, 0.999), np.full(n_back, 0.6), [0.5]]).astype(np.float32)
    n = len(means)
    perm = rng.permutation(n)
    scene = make_scene(means[perm], scales[perm], opac=opac[perm], seed=43)
    return scene, onp.Camera(16, 16, f, f, c, c, EYE.copy()), int(np.nonzero(perm == n - 1)[0][0])


def case_deep_window_ends(drv, survivor="last"):
    """The deep-tile cull's window whose LAST record (survivor='last') or FIRST record ('first') is the only one that reaches a live pixel.
    From the oracle alone: the survivor is the last record of the tile's queue / the first behind the three front layers; the frame without
    it equals the frame of the front layers alone on every pixel (no other back record changes a pixel), and the survivor changes pixels
    of the hole only.  The library (the stats=False instantiation, the one that culls): n_deep_windows > 0 and the oracle's frame
    (check_against_oracle, which also holds it against the instantiation that never culls, bit for bit).
    The twin — the survivor moved off the hole: a window with no survivor at all — n_deep_windows > 0 again and the frame of the front layers."""
    n_front = 3 * (256 - 25)
    for twin in (False, True):
        scene, cam, sid = deep_window_scene(survivor, twin)
        tag = f"deep window ends [{survivor}{', twin' if twin else ''}]"
        ref, aux = oracle_c.render(*scene, cam)
        ids = aux["ids"]
        assert aux["gx"] == aux["gy"] == 1 and aux["D"] == len(scene[0]) <= 1024
        assert ids[-1 if survivor == "last" else n_front] == sid, f"{tag}: the survivor is not where the case wants it in the queue"
        keep = np.arange(len(scene[0])) != sid
        without = tuple(a[keep] for a in scene[:5]) + (0,)
        ref_wo, _ = oracle_c.render(*without, cam)
        z = scene[0][:, 2]
        front_only = tuple(a[z < 1.5] for a in scene[:5]) + (0,)
        ref_front, aux_front = oracle_c.render(*front_only, cam)
        assert np.array_equal(ref_wo, ref_front), f"{tag}: a back record other than the survivor changes a pixel"
        # the live pixels behind the front layers: those that a sheet over the whole tile, put behind them, still changes
        sheet = make_scene(np.array([[0.0, 0.0, 50.0]], np.float32), np.full((1, 3), 500.0), opac=0.9, seed=44)
        with_sheet = tuple(np.concatenate([a, b]) for a, b in zip(front_only[:5], sheet[:5])) + (0,)
        live = np.abs(oracle_c.render(*with_sheet, cam)[0] - ref_front).max(axis=-1) > 0
        hole = np.zeros((16, 16), bool); hole[HOLE] = True
        assert (live == hole).all(), f"{tag}: the live pixels behind the front layers are not the hole"
        changed = np.abs(ref - ref_wo).max(axis=-1) > 0
        if twin:
            assert not changed.any(), f"{tag}: the twin's survivor changes a pixel"
        else:
            assert changed.any() and not (changed & ~hole).any() and np.abs(ref - ref_wo).max() > 0.05, f"{tag}: the survivor does not show in the hole alone"
        img, st, aux2, _ = pc.check_against_oracle(drv, scene, cam, what=tag)
        assert st["n_deep_windows_plain"] > 0, f"{tag}: no window was culled against the live pixels"
        plain, st_plain = drv.render(cam, stats=False, fine=False)
        assert st_plain["n_deep_windows"] > 0
        d = np.abs(plain.astype(np.float64) - ref)[hole].max()
        assert d < 1.0e-3, f"{tag}: the hole differs from the oracle's by {d:.3e} (the survivor contributes up to {np.abs(ref - ref_wo).max():.3f})"
