"""The parity checks must see a kernel that is slightly wrong (CPU, wave64 emulator).

Each mutant is csrc/ with one small textual change — a kernel that is wrong by a few 1e-4 per pixel, or in a few pixels only — built as an
emulator library of its own (never for gfx950).  Its cases run through parity_cases.check_against_oracle twice: with the flat 1e-3 checks
alone, which must PASS (the gap tight_parity.py closes: otherwise the mutant proves nothing), and with tight_parity's budget, which must
FAIL with a [tight] assertion — not with a crash, not with another check.  The anchor of every patch must be found exactly once, so that a
refactor of the kernels cannot make a mutant vanish silently.
"""
import numpy as np
import pytest

import conftest
import emu_harness
import oracle_np as onp
import parity_cases as pc

R11 = "#define SGS_MUT_R11(x) ((x) * 8193.0f - ((x) * 8193.0f - (x)))   /* x rounded to an 11-bit significand: fp16 precision */\n"

INCLUDE = '#include "sgs_common.h"\n'
DEFINE_R11 = (INCLUDE, INCLUDE + R11)                      # every mutant's first edit: the macro, behind the kernels' first include
K = "sgs_kernels.h"
# mutant -> {file of csrc/: [(anchor, replacement)]}
MUTANTS = {
    # SGS_STAGE: the splat's colour staged at fp16 precision
    "stage_rgb_fp16": {K: [DEFINE_R11, ("s_p3[J] = make_float2(B_.z, B_.w);", "s_p3[J] = make_float2(SGS_MUT_R11(B_.z), SGS_MUT_R11(B_.w));"),
                                       ("s_p4[J] = make_float2(C_.x, C_.y);", "s_p4[J] = make_float2(SGS_MUT_R11(C_.x), C_.y);")]},
    # SGS_APPLY: the depth added to the AUX output's expected depth at fp16 precision
    "aux_depth_fp16": {K: [DEFINE_R11, ("if (AUX) Dz = __builtin_fmaf(wgt, (N##4).y, Dz);", "if (AUX) Dz = __builtin_fmaf(wgt, SGS_MUT_R11((N##4).y), Dz);")]},
    # SGS_ALPHA_F: every alpha 2^-13 too large
    "alpha_x(1+2^-13)": {K: [DEFINE_R11, ("AL = SGS_SAT(SGS_EXP2(-q)) * SGS_SAT(__builtin_fmaf(-q, big, cq_big));",
                                          "AL = SGS_SAT(SGS_EXP2(-q)) * SGS_SAT(__builtin_fmaf(-q, big, cq_big)) * (1.0f + 0x1p-13f);")]},
    # fine tiles only: the splat's centre 2^-10 px off along x when the frame is rendered through 8x8 / 4x4-pixel tiles
    "fine_centre_2^-10px": {K: [DEFINE_R11, ("sp[0] = make_float4(sx * up, sy * up,", "sp[0] = make_float4((sx + (zf > 0 ? 0x1p-10f : 0.0f)) * up, sy * up,")]},
    # termination: the stop rule T (1 - alpha) < t_min at 1.05 t_min
    "t_min_x1.05": {K: [DEFINE_R11, ("nt_big = -(P.alpha_max * P.t_min) * SGS_BIG;", "nt_big = -(P.alpha_max * (P.t_min * 1.05f)) * SGS_BIG;")]},
    # background: the final transmittance rounded to fp16 precision before T * bg
    "bg_T_fp16": {K: [DEFINE_R11, ("o[0] = C0 + Tf * P.bg[0]; o[1] = C1 + Tf * P.bg[1]; o[2] = C2 + Tf * P.bg[2];",
                                   "o[0] = C0 + SGS_MUT_R11(Tf) * P.bg[0]; o[1] = C1 + SGS_MUT_R11(Tf) * P.bg[1]; o[2] = C2 + SGS_MUT_R11(Tf) * P.bg[2];")]},
    # the final transmittance of a STOPPED pixel (1 - the sum of its weights) dropped: such a pixel loses T_final bg, between t_min and
    # t_min / (1 - alpha) of the background for the alpha it stopped on — 1.0e-4 to 1.012e-4 in a queue of faint splats (alpha <= 0.012)
    "tf_stopped_zero": {K: [DEFINE_R11, ("const float Tf = Tm > 0.0f ? Tm / amax : fmaxf(1.0f - Wsum, 0.0f);", "const float Tf = Tm > 0.0f ? Tm / amax : 0.0f;")]},
    # SGS_APPLY: the weights summed into 1 - T_final at fp16 precision.  Caught where pixels stop on a few LARGE weights (the deep-tile
    # scene's opaque layers: a weight of 0.99 rounded to 11 bits is off by up to 2.4e-4, the budget there is A = 1.5e-5).  NOT caught on
    # the big-depth-bucket scene, measured under the emulator: ~1100 weights of <= 0.012 rounded to 11 bits move coverage by 4.9e-5,
    # and the budget at n_px = 1100 is A + B n_px = 8.1e-5 — B grants every record one whole rounding of a sum of 1, a faint record's
    # fp16 rounding (w 2^-12 <= 3e-6 each, signs random) stays below that.  The budget is a bound on fp32 arithmetic, not a detector of
    # every lower precision: in a queue of faint records it cannot tell fp16 weights from fp32 ones.
    "tf_wsum_fp16": {K: [DEFINE_R11, ("if (TF) Wsum += wgt;", "if (TF) Wsum += SGS_MUT_R11(wgt);")]},
}
# No mutant sits in the deep-tile branch of render_tile (`!STATS && deep_ok && ...`) alone: that branch culls a window's records against the
# live pixels and compacts the survivors' keys — it holds no line that touches Wsum or Dz; the survivors are staged and blended by the code
# every tile runs (SGS_APPLY, mutated above).  A record it dropped or repeated would show in the colours as well, which case_deep_tile
# holds against the ordinary path bit for bit; check_variants_against_oracle proves that the branch RAN in the TF and AUX kernels.


def _variants(scene_cam, bg=pc.BG, what=""):
    def case(drv):
        scene, cam = scene_cam
        drv.upload(*scene)
        pc.check_variants_against_oracle(drv, scene, cam, bg=bg, what=what, switches=False)
    return case


def _tf_over_white(drv):
    """The TF frame alone (cfg.bg = 1) of the big-depth-bucket scene: every pixel stops, on a faint splat, thousands of records in."""
    import oracle_c
    scene, cam = pc.big_depth_bucket_scene(1500)
    cfg = pc.with_background(None, (1.0, 1.0, 1.0))
    drv.upload(*scene)
    ref, o = oracle_c.render(*scene, cam, cfg, want="image")
    assert float((o["final_T"] < 1.02e-4).mean()) > 0.9, "the pixels of this case are meant to stop"
    for kw in (dict(fine=False), dict()):
        with pc.forced_fine(drv):
            img, _ = drv.render(cam, cfg, stats=False, **kw)
        conftest.assert_frame_close(img, ref, o["margin"], o["recheck"], what=f"big depth bucket over white {kw}")
        pc.assert_frame_tight(img, ref, o, what=f"big depth bucket over white {kw}")


def _fuzz(seeds):
    return lambda drv: pc.case_fuzz(drv, seeds, thorough_every=1 << 30)


def _config1(drv, n=3000):
    scene, cam = onp.config1_scene(n=n, seed=0)          # 128x128, dense enough that pixels stop (T (1 - alpha) < t_min)
    pc.check_against_oracle(drv, scene, cam, what=f"config1 n={n}", thorough=False)


# mutant -> its cases (small frames; thorough=False: the switches that only hold one render against another are left to the main suite)
CASES = {
    "stage_rgb_fp16": _fuzz([1]),
    "aux_depth_fp16": lambda drv: pc.case_depth_aux(drv, n=600, res=(64, 48)),
    "alpha_x(1+2^-13)": _config1,
    "fine_centre_2^-10px": _fuzz([1]),
    "t_min_x1.05": _config1,
    "bg_T_fp16": _fuzz([1]),
    "tf_stopped_zero": _tf_over_white,
    "tf_wsum_fp16": _variants(pc.deep_tile_scene(2000), what="deep tile"),
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("mutants"), MUTANTS, "libsage_gs_mutant.so")


def _run(lib_path, case, tight, monkeypatch):
    """Run `case` on the mutant; tight=False: the tight_parity checks are switched off (today's suite).  Returns the worst |d| the
    flat checks saw (conftest.PARITY_LOG) and the worst depth / coverage |d| of the AUX renders."""
    seen = {"aux": 0.0}
    if not tight:
        def no_tight(*a, **k):
            return 0.0

        def aux_seen(out_aux, o, what=""):
            safe = o["margin"] >= conftest.MARGIN
            d = np.abs(out_aux[..., 0] - o["depth_image"]) / max(1.0, float(o["depth_image"].max()))
            c = np.abs(out_aux[..., 1] - (1.0 - o["final_T"]))
            seen["aux"] = max(seen["aux"], float(d[safe].max(initial=0.0)), float(c[safe].max(initial=0.0)))
            return 0.0, 1.0 - float(safe.mean())
        monkeypatch.setattr(pc, "assert_frame_tight", no_tight)
        monkeypatch.setattr(pc, "assert_depth_coverage_tight", aux_seen)
        monkeypatch.setattr(pc, "assert_aux_tilings_agree", no_tight)
    n0 = len(conftest.PARITY_LOG)
    drv = emu_harness.EmuRenderer(record_capacity=1 << 20, lib_path=lib_path)
    try:
        case(drv)
    finally:
        drv.close()
        monkeypatch.undo()
        rows = conftest.PARITY_LOG[n0:]
        del conftest.PARITY_LOG[n0:]                  # (a mutant's frames stay out of the suite's parity ledger)
    return max([r[3] for r in rows] + [r[4] for r in rows] + [0.0]), seen["aux"]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_passes_the_flat_check_and_fails_the_budget(mutant_libs, name, monkeypatch):
    worst, worst_aux = _run(mutant_libs[name], CASES[name], False, monkeypatch)
    print(f"[mutant] {name}: passes the 1e-3 checks, worst |d| {worst:.2e} (depth / zmax, coverage {worst_aux:.2e})")
    with pytest.raises(AssertionError) as e:
        _run(mutant_libs[name], CASES[name], True, monkeypatch)
    assert str(e.value).startswith("[tight]"), f"{name}: failed, but not on the tight budget: {e.value}"
    print(f"[mutant] {name}: caught: {str(e.value)[:160]}")
