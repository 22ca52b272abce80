"""Seeded faults in the image similarity (csrc/sgs_similarity.h, and the launch in csrc/sgs_api.hip), under the wave64 emulator: each
is made in a copy of csrc/, compiled, and must be caught by similarity_cases' checks — by the assertion named for it.  A copy whose
only change is SGS_SIM_MAX_FRAMES = 4 is compiled beside them: the split of a call into launches, which no seeded fault concerns."""
import re

import pytest

import emu_harness
import similarity_cases as sc
from sage_gs import _capi

H, API = "sgs_similarity.h", "sgs_api.hip"
SPLIT_CHUNK = 4
MUTANTS = {          # name: {file of csrc/: [(anchor, replacement)]}
    "tap_changed_on_one_side": {H: [("{2, 16, 74, 224, 436, 544, 436, 224, 74, 16, 2}", "{2, 17, 74, 224, 436, 544, 436, 224, 74, 16, 2}")]},
    "window_starts_one_late": {H: [("const int px = x0 + lx;", "const int px = x0 + lx + 1;")]},
    "c1_used_for_c2": {H: [("const long long c1 = SGS_SIM_C1, c2 = SGS_SIM_C2;", "const long long c1 = SGS_SIM_C1, c2 = SGS_SIM_C1;")]},
    "covariance_term_unsigned": {H: [("((double)n1 * (double)n2)", "((double)n1 * (double)(unsigned long long)n2)")]},
    "q_by_truncation": {H: [("return (long long)floor(v);", "return (long long)v;")]},
    "second_moment_in_32_bits_vertically": {H: [("return acc + (unsigned long long)w * v;", "return acc + (unsigned long long)(w * v);")]},
    "last_tile_column_dropped": {API: [("const int tiles_x = (nwx + SGS_SIM_TILE_W - 1) / SGS_SIM_TILE_W;", "const int tiles_x = nwx / SGS_SIM_TILE_W;")]},
    "shared_target_stride_ignored": {H: [("const unsigned char* tgt = J.target + f * J.target_stride;",
                                         "const unsigned char* tgt = J.target + f * (J.target_stride ? J.target_stride : 3ll * J.W * J.H);")]},
    "clear_skipped": {API: [("hipLaunchKernelGGL(sgs::k_sim_clear, dim3(clear_blocks), dim3(SGS_SIM_THREADS), 0, st, J);", "(void)clear_blocks;")]},
    "sse_over_windows": {H: [("const bool owned = in && (lx < SGS_SIM_TILE_W || last_x) && (ly < SGS_SIM_TILE_H || last_y);",
                             "const bool owned = in && lx < SGS_SIM_TILE_W && ly < SGS_SIM_TILE_H && px < nwx && py < nwy;")]},
}
SPLIT = {H: [("#define SGS_SIM_MAX_FRAMES 65535 ", f"#define SGS_SIM_MAX_FRAMES {SPLIT_CHUNK} ")]}      # (no fault)
# The first failing assertion of the checks below on each mutant (the values are deterministic).
CAUGHT_BY = {
    "tap_changed_on_one_side": r"11x11 noise_pair: ssim_q is ",            # (identical pictures score 1 under any window)
    "window_starts_one_late": r"11x11 noise_pair: ssim_q is ",
    "c1_used_for_c2": r"11x11 noise_pair: ssim_q is ",
    "covariance_term_unsigned": r"11x11 noise_pair: ssim_q is ",
    "q_by_truncation": r"11x11 noise_pair: ssim_q is \[-49570137, -182177782, -221190410\], the restatement has \[-49570138, -182177783, -221190411\]",
    "second_moment_in_32_bits_vertically": r"11x11 noise_pair: ssim_q is ",
    "last_tile_column_dropped": r"11x11 identical: ssim_q is \[0, 0, 0\]",
    "shared_target_stride_ignored": r"B = 3, shared target: frame 1: ssim_q is ",
    "clear_skipped": r"11x11 identical: the row was not written whole",
    "sse_over_windows": r"11x11 noise_pair: sse is ",
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library and the copy with launches of 4 frames, compiled side by side (one g++ each)."""
    root = tmp_path_factory.mktemp("similarity_mutants")
    split, proc = emu_harness.start_emu_copy(root / "split", SPLIT, "libsage_gs_similarity_split.so")
    libs = emu_harness.build_mutants(root, MUTANTS, "libsage_gs_similarity_mutant.so")
    assert proc.wait() == 0, "split_chunk_4: the copy does not compile"
    libs["split_chunk_4"] = split
    return libs


def _checks(d):
    for shape in sc.SHAPES:
        sc.check_shape(d, shape)
    sc.check_batches(d)


@pytest.mark.parametrize("name", list(CAUGHT_BY))
def test_similarity_mutant_is_caught(mutant_libs, name):
    d = sc.AbiSimilarity(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        _checks(d)
    except AssertionError as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: the similarity's checks pass on this mutant"
    print(f"[similarity mutant] {name}: caught: {str(caught)[:200]}")
    assert re.search(CAUGHT_BY[name], str(caught)), f"{name}: failed on another assertion: {str(caught)[:300]}"


def test_the_unmutated_library_passes_the_mutants_checks():
    d = sc.AbiSimilarity(_capi.Lib(emu_harness.build_emu()))
    try:
        _checks(d)
    finally:
        d.close()


def test_split_launch_with_chunks_of_4_frames(mutant_libs):
    """sgs_image_similarity cuts n_frames into launches of SGS_SIM_MAX_FRAMES (gridDim.y): with the constant at 4, 11 frames take two
    full launches and a short one; then the batches of 1, 3 and 9 frames, the last of which is cut 4 + 4 + 1."""
    d = sc.AbiSimilarity(_capi.Lib(mutant_libs["split_chunk_4"]))
    try:
        assert sc.check_split(d, SPLIT_CHUNK) == 2 * SPLIT_CHUNK + 3
        sc.check_batches(d)
    finally:
        d.close()
