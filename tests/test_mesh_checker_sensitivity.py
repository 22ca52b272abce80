"""The collision-mesh depth checks must see a mesh kernel that is slightly wrong (CPU, wave64 emulator).

As test_checker_sensitivity.py does for the splat path: each mutant is csrc/ with one small textual change to sgs_mesh.h, built as an
emulator library of its own (never for gfx950), and the mesh case that targets it must fail with an AssertionError — not a crash, not a
refusal.  The anchor of every patch must be found exactly once, so that a refactor of the kernels cannot make a mutant vanish silently.
"""
import re

import pytest

import emu_harness
import mesh_edge_cases as mc

FMA_CROSS = '''
__device__ __forceinline__ MeshD3 mesh_cross_fma(const MeshD3& a, const MeshD3& b) {
    return MeshD3{fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x))};
}
__device__ __forceinline__ MeshD3 mesh_cross_f32(const MeshD3& a, const MeshD3& b) {
    const float ax = (float)a.x, ay = (float)a.y, az = (float)a.z, bx = (float)b.x, by = (float)b.y, bz = (float)b.z;
    return MeshD3{fmaf(ay, bz, -(az * by)), fmaf(az, bx, -(ax * bz)), fmaf(ax, by, -(ay * bx))};
}
'''
CROSS_ANCHOR = "__device__ __forceinline__ unsigned mesh_tile_of("
EDGE_PLANE = ("const MeshD3 e = swap ? mesh_cross_rn(p[b], p[a]) : mesh_cross_rn(p[a], p[b]);\n"
              "                        const double s = swap ? -sg : sg;")
EDGE_PLANE64 = "const MeshD3 e = mesh_cross_rn(u, v);"             # mesh_inside64's plane (its sign comes from the record)

H = "sgs_mesh.h"
# mutant -> {file of csrc/: [(anchor, replacement)]}
MUTANTS = {
    # an edge on the line through a pixel centre belongs to neither triangle (the fp32 test and its fp64 recheck)
    "exclusive_edges": {H: [("bool in = s0 >= 0.f && s1 >= 0.f && s2 >= 0.f;", "bool in = s0 > 0.f && s1 > 0.f && s2 > 0.f;"),
                            ("if (s[k] >= 0.f) continue;", "if (s[k] > 0.f) continue;"),
                            ("if (!(g >= -0x1p-50 * fma(Px, ax, fma(Py, ay, Pz)))) return false;", "if (!(g > 0.0)) return false;")]},
    # each triangle builds its edge planes in its own vertex order with a fused fp64 cross product (the record and the recheck)
    "fused_cross_triangle_order": {H: [(CROSS_ANCHOR, FMA_CROSS + CROSS_ANCHOR),
                                       (EDGE_PLANE, "const MeshD3 e = mesh_cross_fma(p[a], p[b]);\n                        const double s = sg;"),
                                       (EDGE_PLANE64, "const MeshD3 e = mesh_cross_fma(p[a], p[b]);")]},
    # the same in fp32 (a setup moved to single precision): the two sides of a shared edge differ by an ulp
    "fp32_cross_triangle_order": {H: [(CROSS_ANCHOR, FMA_CROSS + CROSS_ANCHOR),
                                      (EDGE_PLANE, "const MeshD3 e = mesh_cross_f32(p[a], p[b]);\n                        const double s = sg;"),
                                      (EDGE_PLANE64, "const MeshD3 e = mesh_cross_f32(p[a], p[b]);")]},
    # the fp64 recheck of edges within rounding of 0 is gone: a vertex's fan can leave its pixel unclaimed
    "no_fp64_recheck": {H: [("if (!in && fmaf(e0.w, rmax,", "if (false && fmaf(e0.w, rmax,")]},
    "far_exclusive": {H: [("if (z > near_z && z <= far_z) best", "if (z > near_z && z < far_z) best")]},
    "near_inclusive": {H: [("if (z > near_z && z <= far_z) best", "if (z >= near_z && z <= far_z) best")]},
    # k_mesh_scan: the running sum of the blocks before is not carried into the next block of 1024 tiles
    "scan_carry_lost": {H: [("const unsigned carry = s_carry;", "const unsigned carry = 0u * s_carry;")]},
    # k_mesh_depth: only the first LDS chunk (256 records) of a tile's list is read
    "first_chunk_only": {H: [("for (unsigned long long b = begin; b < end; b += 256) {", "for (unsigned long long b = begin; b < end; b = end) {")]},
}


def _exact_lattice(drv):
    mc.check_edge_case(drv, "lattice_exact", 128, 96, seed=1)


def _inexact_lattices(drv):
    for seed, (w, h) in enumerate([(128, 96), (200, 136), (256, 192)]):
        mc.check_edge_case(drv, "lattice_inexact", w, h, seed=seed)


def _vertex_pixels(drv):
    for seed in (128, 5, 6):
        mc.check_edge_case(drv, "lattice_inexact", 128, 96, seed=seed)


CASES = {
    "exclusive_edges": _exact_lattice,
    "fused_cross_triangle_order": _inexact_lattices,
    "fp32_cross_triangle_order": _inexact_lattices,
    "no_fp64_recheck": _vertex_pixels,
    "far_exclusive": mc.case_near_far_exact,
    "near_inclusive": mc.case_near_far_exact,
    "scan_carry_lost": mc.case_many_tiles,
    "first_chunk_only": mc.case_many_tiles,
}

# what the failure must say: the check that is meant to catch the mutant, not a guard of the case's own setup
CAUGHT_BY = {
    "exclusive_edges": r"\(edge-exact\).*must claim",
    "fused_cross_triangle_order": r"\(edge-exact\).*must claim",
    "fp32_cross_triangle_order": r"\(edge-exact\).*must claim",
    "no_fp64_recheck": r"\(edge-exact\).*must claim",
    "far_exclusive": r"quad at z == far_z: not visible",
    "near_inclusive": r"row at z == near_z",
    "scan_carry_lost": r"outside \[lenient, strict\]|differ from the band",
    "first_chunk_only": r"outside \[lenient, strict\]|differ from the band",
}

# measured: fp64 products differ in the last bits only, and rounding e to fp32 hides that at every edge of the lattices above — both
# triangles of an edge still evaluate +-the same fp32 plane, and the fp64 recheck's margin (2^-50) is far above that difference.  The fp32
# variant (next mutant) is the one a rewrite would make.
XFAIL = {"fused_cross_triangle_order": "the fused fp64 cross product rounds to the same fp32 edge plane as the unfused one: no crack"}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("mesh_mutants"), MUTANTS, "libsage_gs_mesh_mutant.so")


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=XFAIL[n]))
                                  if n in XFAIL else n for n in MUTANTS])
def test_mesh_mutant_is_caught(mutant_libs, name):
    from sage_gs import _capi
    drv = mc.EmuMesh(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        CASES[name](drv)
    except AssertionError as e:
        caught = e
    finally:
        drv.close()
    assert caught is not None, f"{name}: no mesh check fails on this mutant"
    assert re.search(CAUGHT_BY[name], str(caught)), f"{name}: failed on another assertion: {str(caught)[:300]}"
    print(f"[mesh mutant] {name}: caught: {str(caught)[:200]}")
