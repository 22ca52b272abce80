"""A per-pixel error budget for oracle-checked frames, next to conftest.assert_frame_close's flat 1e-3.

The kernels and the oracle (fp64 blend of the same fp32 splats) differ by a few 1e-7 per pixel, 1e-6 at worst; the flat 1e-3 lets a kernel
that is wrong by a few 1e-4 (a colour staged at fp16 precision, an alpha off by 2^-13, a pixel centre off by 2^-10 px) pass.  Here every
pixel is held to

    tol_px = A + B * n_px,        n_px = aux["n_contrib"]: one more than the queue position of the last pair the oracle blended

Budget, in u = 2^-24 (fp32 rounding); colours below c_max ~ 2 in these scenes; the oracle blends the kernel's own fp32 splats in fp64.
  * A, what does not grow with the queue.  Each alpha: the completed square q = U^2 + (V^2 + nlo) is five fmas over terms below
    cq = log2(alpha_max / alpha_min) < 10, the roots (a, a k, c) and the fp32 conic under them are 1 ulp each, exp2 (v_exp_f32) 1 ulp:
    |d alpha| / alpha < ln2 (5 * 16 u + 2 * 10 u) + u ~ 70 u.  Such an error moves weight between a record and those behind it, but
    w and T move together (sum w + T = 1 on both sides), so the colour moves by at most c_max * 70 u ~ 8e-6 in all; the final T * bg
    and the splat's fp32 colour (the oracle's fp64 SH sum, rounded) add a few u.  A = 2^8 u = 1.5e-5.
  * B, per queue position up to the last blended pair: T (1 - alpha), w = alpha T and the colour fmas round once each; one unit
    rounding per record, B = u = 6e-8 (the errors of successive records do not line up: the suites show a slope of ~2e-9 per record).
The splat checks of check_against_oracle grant a conic 1e-5 and a colour 2e-5; a kernel that used that much would move pixels by up to
~1e-4 and fail here.  They are tolerances of those checks, not errors the kernels make (both sides round the same fp64 values to fp32):
in practice the splats agree to an ulp, and a pixel over this budget is a finding to explain, not a reason to widen A or B.
Measured (the [tight] lines), worst err / tol_px: 0.05 on the CPU (emulator) suite, 0.07 on the GPU suite (437 frames, 1.6e8 pixels;
off-threshold worst |d| 1e-6 at n_px < 16, 2e-6 at n_px >= 64); depth / coverage 0.04.  That is the >= 5x headroom the budget keeps.
The TF and AUX instantiations (parity_cases.check_variants_against_oracle: a background of (0.25, 0.5, 0.75), sgs_render_rgbd) on the
stress cases and at the BASELINE sizes, worst err / tol_px: frames over a background 0.026 (emulator, 27 scenes) / 0.037 (GPU, 33 scenes up
to 3 M Gaussians at 3840x2160), depth / coverage 0.040 / 0.043; at most 2.4 % of a frame near a threshold (the cap is 5 %).  The long sum
1 - sum w of a stopped pixel (big depth bucket: ~1100 adds of w <= 0.012) stays at 0.03 of its budget: every add rounds to half an ulp
of a sum below 1, n 2^-25 at worst, and the errors do not line up.

Threshold-sensitive pixels (margin < MARGIN) whose error exceeds tol_px go through aux["recheck"] (every admissible set of alpha cut-off /
stop decisions): the best variant must be within tol_px.  A pixel whose recheck is `capped` (more decisions in the margin than the
oracle enumerates) keeps only conftest's 1e-3 check; such pixels are counted.  (Flagged pixels above RECHECK of their budget are
rechecked too, so that the worst err / tol_px reported is the distance to the nearest admissible evaluation, not to the nominal one.)
"""
import numpy as np

from conftest import MARGIN

U = 2.0 ** -24
A = 2.0 ** 8 * U    # per pixel (1.5e-5)
B = U               # per queue position up to the last blended pair
A_Z, B_Z = A, B     # depth (sum T alpha z), as a fraction of the depth of the pixel's last blended splat

RECHECK = 0.05      # flagged pixels above this fraction of their budget are checked two-sidedly
N_EDGES = (0, 1, 4, 16, 64, 256, 1024, 1 << 62)      # n_px buckets of the per-frame distribution
TIGHT_LOG = []      # one entry per checked frame: (what, pixels, worst ratio, flagged, rechecked, capped, {bucket: (pixels, worst |d|)})


def budget(n_px, a=A, b=B):
    return a + b * np.asarray(n_px, np.float64)


def _distribution(err, n):
    out = {}
    k = np.searchsorted(np.asarray(N_EDGES[1:]), n, side="right")
    for i in range(len(N_EDGES) - 1):
        sel = k == i
        if sel.any():
            out[N_EDGES[i]] = (int(sel.sum()), float(err[sel].max()))
    return out


def assert_frame_tight(img, ref, aux, y0=0, what="frame"):
    """|img - ref| <= A + B n_px on every pixel of img (a band of the frame starting at pixel row y0, or the frame): call it right after
    the assert_frame_close it strengthens, with the oracle's aux of the same frame (n_contrib, margin, recheck — full-frame arrays).
    Returns the worst err / tol_px over the pixels held to the budget."""
    img = np.asarray(img, np.float64); ref = np.asarray(ref, np.float64)
    H = img.shape[0]
    n = np.asarray(aux["n_contrib"])[y0:y0 + H]
    margin = np.asarray(aux["margin"])[y0:y0 + H]
    assert n.shape == img.shape[:2] == margin.shape, (what, n.shape, img.shape, margin.shape)
    err = np.abs(img - ref).max(axis=-1)
    tol = budget(n)
    ratio = err / tol
    safe = margin >= MARGIN
    over = safe & ~(err <= tol)
    if over.any():
        ys, xs = np.nonzero(over)
        i = int(np.argmax(ratio[over]))
        raise AssertionError(f"[tight] {what}: {len(ys)} pixel(s) with no decision near a threshold exceed A + B n_px: worst |d| "
                             f"{err[ys[i], xs[i]]:.3e} = {ratio[ys[i], xs[i]]:.1f} x budget at (y,x)=({ys[i] + y0},{xs[i]}), n_px {n[ys[i], xs[i]]}")
    worst = float(ratio[safe].max(initial=0.0))
    flagged = ~safe
    # a flagged pixel's nominal error says nothing about the kernel when one of its decisions went the other way (it is then the size of
    # the flipped contribution, anywhere from 0 up): every flagged pixel above RECHECK of its budget is held to its best variant
    ys, xs = np.nonzero(flagged & ~(err <= RECHECK * tol))
    n_over = n_capped = 0
    big = ""
    if len(ys):
        recheck = aux.get("recheck")
        assert recheck is not None, f"[tight] {what}: {len(ys)} threshold-sensitive pixels need a two-sided check and no oracle for it was supplied"
        best, leaves, capped = recheck(ys + y0, xs, img[ys, xs])
        best = np.asarray(best, np.float64); capped = np.asarray(capped, bool)
        t = tol[ys, xs]; e = err[ys, xs]
        over = ~(e <= t)
        n_over, n_capped = int(over.sum()), int((capped & over).sum())
        bad = over & ~capped & ~(best <= t)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"[tight] {what}: {int(bad.sum())} threshold-sensitive pixel(s) match no admissible evaluation within "
                                 f"A + B n_px: best |d| {best[i]:.3e} (budget {t[i]:.3e}) at (y,x)=({ys[i] + y0},{xs[i]}), n_px {n[ys[i], xs[i]]}, "
                                 f"{int(leaves[i])} variants")
        held = ~(over & capped)
        if held.any():
            worst = max(worst, float((np.minimum(e, best)[held] / t[held]).max()))
        i = int(np.argmax(e))
        big = f"; largest flagged |d| {e[i]:.2e} at (y,x)=({ys[i] + y0},{xs[i]}) n_px {n[ys[i], xs[i]]}: best of {int(leaves[i])} variants {best[i]:.2e}"
    rest = flagged & (err <= RECHECK * tol)
    worst = max(worst, float(ratio[rest].max(initial=0.0)))
    dist = _distribution(err[safe], n[safe])
    TIGHT_LOG.append((what, int(err.size), worst, int(flagged.sum()), n_over, n_capped, dist))
    print(f"[tight] {what}: {err.size} px, worst err/tol_px {worst:.3f} (A {A:g}, B {B:g}), {int(flagged.sum())} flagged, "
          f"{len(ys)} rechecked ({n_over} over the budget), {n_capped} capped; off-threshold worst |d| by n_px: "
          + " ".join(f"{k}+:{v[1]:.1e}/{v[0]}" for k, v in dist.items()) + big)
    return worst


def depth_coverage_budgets(o):
    """(depth budget [H, W], coverage budget [H, W], pixels with no decision near a threshold [H, W]) of the oracle's full-frame `o`."""
    n = np.asarray(o["n_contrib"]).astype(np.int64)
    H, W = n.shape
    safe = np.asarray(o["margin"]) >= MARGIN
    gx = (W + 15) // 16
    yy, xx = np.mgrid[0:H, 0:W]
    tile = (yy // 16) * gx + xx // 16
    last = o["offsets"][tile] + n - 1
    z_all = o["depth_bits"].view(np.float32)
    zpx = np.where(n > 0, z_all[o["ids"][np.clip(last, 0, max(0, len(o["ids"]) - 1))]] if len(o["ids"]) else 0.0, 1.0).astype(np.float64)
    return budget(n, A_Z, B_Z) * zpx, budget(n), safe


def assert_depth_coverage_tight(out_aux, o, what="frame"):
    """The depth / coverage outputs of an AUX render (out_aux [H, W, 2]: sum T alpha z, 1 - T_final) against the oracle's full-frame
    `o` (want="all": its queues give each pixel's depth scale).  Depth: (A_Z + B_Z n_px) times the depth of the pixel's last blended splat
    (queues run in ascending depth, so every blended z is at most that); coverage: the colour budget (a colour of 1).  Pixels with a
    decision near a threshold keep only the existing checks.  Returns (the worst ratio of the two, the share of the frame's pixels that
    were skipped for that reason) — a caller that leans on this check bounds the share, so that "all pixels skipped" cannot pass."""
    n = np.asarray(o["n_contrib"]).astype(np.int64)
    tz, tc, safe = depth_coverage_budgets(o)
    dz = np.abs(out_aux[..., 0].astype(np.float64) - o["depth_image"])
    cov = np.abs(out_aux[..., 1].astype(np.float64) - (1.0 - o["final_T"].astype(np.float64)))
    for name, e, t in (("depth", dz, tz), ("coverage", cov, tc)):
        over = safe & ~(e <= t)
        if over.any():
            ys, xs = np.nonzero(over)
            i = int(np.argmax((e / t)[over]))
            raise AssertionError(f"[tight] {what}: {name}: {len(ys)} pixel(s) exceed the budget: worst |d| {e[ys[i], xs[i]]:.3e} "
                                 f"(budget {t[ys[i], xs[i]]:.3e}) at (y,x)=({ys[i]},{xs[i]}), n_px {n[ys[i], xs[i]]}")
    wz = float((dz / tz)[safe].max(initial=0.0)); wc = float((cov / tc)[safe].max(initial=0.0))
    skipped = 1.0 - float(safe.mean()) if safe.size else 0.0
    print(f"[tight] {what} depth/coverage: worst err/tol_px {wz:.3f} / {wc:.3f} over {int(safe.sum())} px ({100 * skipped:.2f} % of the frame skipped: near a threshold)")
    return max(wz, wc), skipped


def assert_aux_tilings_agree(aux_a, aux_b, o, what="frame"):
    """Depth / coverage of one frame through two tilings (another tile origin: not the same bits, as for RGB).  Each is held to the oracle
    `o` within the budget, so on the pixels with no decision near a threshold they are within twice the budget of each other."""
    tz, tc, safe = depth_coverage_budgets(o)
    d = np.abs(np.asarray(aux_a, np.float64) - np.asarray(aux_b, np.float64))
    bad = safe & ~((d[..., 0] <= 2.0 * tz) & (d[..., 1] <= 2.0 * tc))
    if bad.any():
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"[tight] {what}: depth / coverage differ between two tilings by more than twice the budget in {len(ys)} pixel(s), "
                             f"first at (y,x)=({ys[0]},{xs[0]}): |d| {d[ys[0], xs[0], 0]:.3e} / {d[ys[0], xs[0], 1]:.3e}")
