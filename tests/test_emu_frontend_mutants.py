"""Seeded faults in the splat renderer's front end and sort (csrc/sgs_kernels.h: the projection, the cheap exclusion, the chunk cull, the bin
and quadrant extents, the tie handling of the HBM sort, the deep-tile cull), under the wave64 emulator: each is made in a copy of csrc/,
compiled, and must be caught by the ONE case named for it — by the assertion named for it; a crash or another check does not count.

Four of these faults passed every case the emulator suite had before frontend_cases.py (both chunk-cull margins, the far plane, the first
record of a short tie run); six more were caught only by whichever fuzz seed happened to land on them.  Their cases are now the
deterministic ones of frontend_cases.py.  Mutants are emulator builds: never compiled for gfx950, never run in a `gpu` test."""
import re

import pytest

import emu_harness
import frontend_cases as fc
import parity_cases as pc

K = "sgs_kernels.h"
MUTANTS = {          # name: [(anchor, replacement)] in csrc/sgs_kernels.h
    # ---- chunk cull (chunk_outside)
    "chunk_sphere_radius_times_0_9": [("const double Rp = R * 1.0001 + 1.0e-6 * (fabs(tx) + fabs(ty) + fabs(tz));", "const double Rp = R * 0.9;")],
    "chunk_scale_allowance_halved": [("const double d = P.cull_A * sm,", "const double d = 0.5 * P.cull_A * sm,")],
    "chunk_near_test_without_the_radius": [("if (tz + Rp < (double)P.near_z ||", "if (tz < (double)P.near_z ||")],
    # ---- projection (preprocess_chunk)
    "far_plane_exclusive": [("tz <= (double)P.far_z;", "tz < (double)P.far_z;")],
    "near_plane_inclusive": [("tz > (double)P.near_z && tz <=", "tz >= (double)P.near_z && tz <=")],
    "cheap_exclusion_without_the_clamp_terms": [("(2.0f + lx * lx + ly * ly)", "(1.0f)")],
    "cheap_exclusion_band_top_8_px_low": [("(float)P.cull_y0 + 1.0f", "(float)P.cull_y0 + 9.0f")],
    "jacobian_clamp_removed_on_x": [("const double txc = fmin(limx, fmax(-limx, xz)) * tz;", "const double txc = xz * tz;")],
    "jacobian_clamp_removed_on_y": [("const double tyc = fmin(limy, fmax(-limy, yz)) * tz;", "const double tyc = yz * tz;")],
    "determinant_in_fp32": [("const double det = a * c - b * b;", "const double det = (double)((float)a * (float)c - (float)b * (float)b);")],
    "radius_floor_of_0_1_removed": [("sqrt(fmax(0.1, mid * mid - det))", "sqrt(fmax(0.0, mid * mid - det))")],
    "bin_extents_times_0_97": [("sqrtf(Kc * wx) * 1.0001f + 0.02f, hy_ = sqrtf(Kc * wy) * 1.0001f + 0.02f;", "sqrtf(Kc * wx) * 0.97f + 0.02f, hy_ = sqrtf(Kc * wy) * 0.97f + 0.02f;")],
    "bin_rect_low_edge_one_pixel_short": [("const float lo_x = ceilf((fpx - hx - epx - cpl) * icp)", "const float lo_x = ceilf((fpx - hx - epx - cpl + 1.0f) * icp)")],
    "quadrant_extents_times_0_97": [("sqrtf(qmax * wx) * 1.01f + 0.5f, ey_ = sqrtf(qmax * wy) * 1.01f + 0.5f;", "sqrtf(qmax * wx) * 0.97f, ey_ = sqrtf(qmax * wy) * 0.97f;")],
    "sh_degree_3_constant_off_by_1e_4": [("0.3731763325901154f", "0.3732763325901154f")],
    "owned_row_rounds_down": [("(F - P.row_phase + P.row_stride - 1) / P.row_stride : 0;", "(F - P.row_phase) / P.row_stride : 0;")],
    "group_cull_without_the_scale_allowance": [("!chunk_outside(P, b0, b1);", "!chunk_outside(P, b0, make_float4(0.f, 0.f, 0.f, 0.f));")],
    "work_list_frame_field_two_bits": [("const FrameSlot& S = G.s[e & 7u];", "const FrameSlot& S = G.s[e & 3u];")],
    # ---- HBM sort (sort_segment) and the deep-tile cull (k_tile_render)
    "tie_fixup_never_moves_a_runs_first_record": [("while (q > i && a_v[q - 1] > v)", "while (q > i + 1 && a_v[q - 1] > v)")],
    "long_tie_run_not_flagged": [("if (e - i > SGS_TIE_RUN_MAX) { atomicOr(&sh.flag, 1u); }", "if (e - i > SGS_TIE_RUN_MAX) { }")],
    "deep_window_drops_its_last_record": [("hv[u] = i < wcnt;", "hv[u] = i + 1 < wcnt;")],
    "deep_window_drops_its_first_record": [("hv[u] = i < wcnt;", "hv[u] = i > 0u && i < wcnt;")],
    "quadrant_extent_test_with_a_wrong_sign": [("ry - hy <= lr.w && ry + hy >= lr.z", "ry + hy <= lr.w && ry + hy >= lr.z")],
    "packed_sh_byte_taken_from_the_next_lane": [("c[3 + j] = sgs_sh_byte((w[3 + (j >> 2)] >> (8 * (j & 3))) & 0xffu);",
                                                 "c[3 + j] = sgs_sh_byte((w[3 + (j >> 2)] >> (8 * ((j + 1) & 3))) & 0xffu);")],
}
def _random_frame(d):
    """A few hundred mid-sized splats through the full comparison: what every extent of the binning is held by."""
    pc.check_against_oracle(d, pc.random_scene(600, 31, 1, scale=(0.05, 0.4)), fc.margin_cameras()["off_centre"], what="random frame")


def _packed_sh_frame(d):
    """A compressed scene (8-bit SH coefficients, dequantised per frame by eval_sh<DEG, true>) against the same file decoded by NumPy and
    uploaded as fp32 arrays: the frames agree to rounding (the quantised geometry is decoded on both sides)."""
    import tempfile
    import numpy as np
    from sage_gs import ply
    rng = np.random.default_rng(12)
    n = 800
    means = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 7, n)], 1).astype(np.float32)
    scales = np.exp(rng.normal(-2.2, 0.5, (n, 3))).astype(np.float32)
    quats = rng.normal(size=(n, 4)); quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    sh = (rng.normal(size=(n, 16, 3)) * 0.3).astype(np.float32)
    cam = fc.margin_cameras()["identity"]
    with tempfile.TemporaryDirectory() as tmp:
        path = tmp + "/c3.ply"
        ply.save_compressed_ply(path, means, scales, quats, rng.uniform(0.05, 1.0, n).astype(np.float32), sh, 3)
        d.upload(*ply.load_compressed_ply(path, sh_decode="bin_centre"))
        ref, st_ref = d.render(cam)
        d.upload_compressed(*ply.read_compressed_payload(path), sh_decode="bin_centre")
        img, st = d.render(cam)
    assert st["n_visible"] == st_ref["n_visible"] and ref.max() > 0.2
    err = float(np.abs(img - ref).max())
    assert err < 2e-4, f"packed SH: the compressed scene's frame differs from the frame of its NumPy decode by {err:.2e}"


BIG_CAP = 3
_CAP_EDIT = {"sgs_common.h": [("#define SGS_BIG_CAP 65536 ", f"#define SGS_BIG_CAP {BIG_CAP} ")]}
# Faults behind a constant that the emulator cannot reach at its product value (65 536 big splats): made in a copy whose constant is small;
# the copy WITHOUT the fault (`control`) must pass the case.  name: (edits of the control, edits of the fault on top)
CONTROLLED = {
    "big_list_overflow_lanes_stay_marked_big": (_CAP_EDIT, {K: [("if (k < SGS_BIG_CAP) big_list[k] = (unsigned)pos; else big = false;",
                                                                 "if (k < SGS_BIG_CAP) big_list[k] = (unsigned)pos;")]}),
}


def _big_list_overflow(d):
    """Eight splats over every tile of a 768x768 frame (144 super-tiles, more than SGS_BIG_RECT) in ONE chunk, under a big-splat list of
    BIG_CAP entries: the wave straddles the cap, the lanes beyond it go down the per-chunk wave path (test_gpu_campaigns.py does this
    at the product's 65 536 on the GPU).  D under reference binning is the sum of the rect areas; the production frame is that frame."""
    import numpy as np
    import oracle_np as onp
    W = 768
    f = 0.9 * W
    rng = np.random.default_rng(2024)
    n_big, n_small = 8, 40
    z = np.concatenate([np.linspace(2.0, 9.0, n_big), rng.uniform(2.0, 20.0, n_small)])
    means = np.stack([rng.uniform(-0.05, 0.05, len(z)) * z, rng.uniform(-0.05, 0.05, len(z)) * z, z], 1)
    scales = np.concatenate([np.repeat((2000.0 * z[:n_big] / f)[:, None], 3, 1), np.full((n_small, 3), 0.02)])
    opac = np.concatenate([np.full(n_big, 0.02), np.full(n_small, 0.5)])
    scene = fc.make_scene(means, scales, opac=opac, seed=1)
    cam = onp.Camera(W, W, f, f, W / 2.0, W / 2.0, np.eye(4, dtype=np.float32))
    d.upload(*scene)
    img, st = d.render(cam, stats=False, fine=False)
    ref, st_ref = d.render(cam, full_sort=True, loose_cull=True)
    _, _, slot_ids, sp = d.intermediates()
    x0, y0, x1, y1 = sp[:, 10] & 0xffff, sp[:, 10] >> 16, sp[:, 11] & 0xffff, sp[:, 11] >> 16
    whole = int(((x0 == 0) & (y0 == 0) & (x1 == 48) & (y1 == 48)).sum())
    assert whole == n_big > BIG_CAP, whole
    area = int(((x1 - x0).astype(np.int64) * (y1 - y0)).sum())
    assert st_ref["d_total"] == area, f"big list overflow: D is {st_ref['d_total']}, the rects of the visible splats add up to {area}"
    assert (img == ref).all() and st["d_total"] >= whole * 48 * 48, "big list overflow: the production frame differs from the reference-binning frame"


CASES = {            # name: (the case, the assertion that must catch the fault)
    "chunk_sphere_radius_times_0_9": (lambda d: fc.case_chunk_margins(d, "identity"), r"frame: chunk 'left' is SKIPPED although its member \d+ is visible"),
    "chunk_scale_allowance_halved": (lambda d: fc.case_chunk_margins(d, "off_centre"), r"frame: chunk 'scale_left' is SKIPPED although its member \d+ is visible"),
    "chunk_near_test_without_the_radius": (lambda d: fc.case_chunk_margins(d, "turned"), r"frame: chunk 'near' is SKIPPED although its member \d+ is visible"),
    "far_plane_exclusive": (fc.case_near_far_equality, r"the library sees z = \['near \+ ulp', 'far - ulp'\], the oracle"),
    "near_plane_inclusive": (fc.case_near_far_equality, r"the library sees z = \['near', 'near \+ ulp', 'far - ulp', 'far'\], the oracle"),
    "cheap_exclusion_without_the_clamp_terms": (lambda d: fc.case_clamped_giants(d, "identity"), r"clamped giants \[identity\]: rows \(0, -1\): the library sees \['band_first_row', 'band_last_row'\], the oracle \['left', "),
    "cheap_exclusion_band_top_8_px_low": (lambda d: fc.case_chunk_margins(d, "identity"), r"rows \(0, -1\): the library sees the Gaussians"),
    "jacobian_clamp_removed_on_x": (lambda d: fc.case_clamped_giants(d, "turned"), r"the tile rect of giant '\w+' is"),
    "jacobian_clamp_removed_on_y": (lambda d: fc.case_clamped_giants(d, "off_centre"), r"the tile rect of giant '\w+' is"),
    "determinant_in_fp32": (fc.case_needle_determinant, r"needle determinant: the library's conic is off by"),
    "radius_floor_of_0_1_removed": (lambda d: fc.case_chunk_margins(d, "identity"), r"rows \(0, -1\): the library sees the Gaussians"),
    "bin_extents_times_0_97": (_random_frame, r"random frame: culling changed the frame"),
    "bin_rect_low_edge_one_pixel_short": (_random_frame, r"random frame: culling changed the frame"),
    "quadrant_extents_times_0_97": (_random_frame, r"random frame: max \|d\| = "),
    "sh_degree_3_constant_off_by_1e_4": (lambda d: pc.check_against_oracle(d, pc.random_scene(300, 23, 3), fc.margin_cameras()["identity"], what="degree 3"), r"degree 3: SH colour"),
    "owned_row_rounds_down": (lambda d: pc.case_interleaved_rows(d, 2, n=600, res=(112, 100)), r"stride 2 phase"),
    "group_cull_without_the_scale_allowance": (lambda d: fc.case_chunk_margins(d, "identity"), r"batch: chunk 'scale_left' is SKIPPED although its member \d+ is visible"),
    "work_list_frame_field_two_bits": (fc.case_batch_groups_of_eight, r"batch groups of eight: frame 4 differs from the frame rendered alone"),
    "tie_fixup_never_moves_a_runs_first_record": (fc.case_short_tie_runs, r"the queue differs from \(depth bits, index\) order at \d+ positions"),
    "long_tie_run_not_flagged": (lambda d: fc.case_short_tie_runs(d, resort=True), r"the queue differs from \(depth bits, index\) order at \d+ positions"),
    "deep_window_drops_its_last_record": (lambda d: fc.case_deep_window_ends(d, "last"), r"deep window ends \[last\]: the frame depends on whether D_f is counted"),
    "deep_window_drops_its_first_record": (lambda d: fc.case_deep_window_ends(d, "first"), r"deep window ends \[first\]: the frame depends on whether D_f is counted"),
    "quadrant_extent_test_with_a_wrong_sign": (_random_frame, r"random frame: max \|d\| = "),
    "packed_sh_byte_taken_from_the_next_lane": (_packed_sh_frame, r"packed SH: the compressed scene's frame differs from the frame of its NumPy decode by"),
}
assert set(MUTANTS) == set(CASES)


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each; every anchor must be found exactly once)."""
    edits = {name: {K: e} for name, e in MUTANTS.items()}
    for name, (control, fault) in CONTROLLED.items():
        edits["control of " + name] = control
        edits[name] = {**control, **fault}
    return emu_harness.build_mutants(tmp_path_factory.mktemp("frontend_mutants"), edits, "libsage_gs_frontend_mutant.so")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_frontend_mutant_is_caught(mutant_libs, name):
    case, pattern = CASES[name]
    d = emu_harness.EmuRenderer(record_capacity=1 << 21, lib_path=mutant_libs[name])
    caught = None
    try:
        case(d)
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: its case passes on this mutant"
    print(f"[frontend mutant] {name}: caught: {str(caught)[:300]}")
    assert re.search(pattern, str(caught)), f"{name}: failed on another assertion: {str(caught)[:400]}"


def test_the_unmutated_library_passes_every_case_of_the_mutants():
    d = emu_harness.EmuRenderer(record_capacity=1 << 21)
    try:
        for name, (case, _) in CASES.items():
            case(d)
    finally:
        d.close()


def test_big_list_overflow_fault_is_caught_and_its_control_passes(mutant_libs):
    name = "big_list_overflow_lanes_stay_marked_big"
    d = emu_harness.EmuRenderer(record_capacity=1 << 21, lib_path=mutant_libs["control of " + name])
    try:
        _big_list_overflow(d)
    finally:
        d.close()
    d = emu_harness.EmuRenderer(record_capacity=1 << 21, lib_path=mutant_libs[name])
    try:
        with pytest.raises(AssertionError) as e:
            _big_list_overflow(d)
    finally:
        d.close()
    print(f"[frontend mutant] {name}: caught: {str(e.value)[:300]}")
    assert re.search(r"big list overflow: D is \d+, the rects of the visible splats add up to \d+", str(e.value)), f"{name}: failed on another assertion: {str(e.value)[:400]}"
