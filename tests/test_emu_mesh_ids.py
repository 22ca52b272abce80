"""Collision-mesh object ids (sgs_render_mesh_ids*) under the wave64 emulator: the product's kernels (csrc/sgs_mesh.h, k_mesh_ids)
through the cases of tests/mesh_id_cases.py, and the checker's own sensitivity.  CPU only; the 2 000-triangle room and small frames."""
import numpy as np
import pytest

import emu_harness as eh
import mesh_id_cases as ic
import mesh_id_ref as idref


@pytest.fixture(scope="module")
def lib():
    return eh.lib()


@pytest.fixture
def emu(lib):
    e = ic.EmuIds(lib)
    yield e
    e.close()


@pytest.mark.parametrize("w,h", [(160, 120), (33, 17)])
def test_room_against_reference(emu, w, h):
    ic.case_reference(emu, 2000, w, h)


def test_known_answer(emu):
    ic.case_known_answer(emu)


def test_tie_rule(emu):
    ic.case_tie_rule(emu)


def test_nearest_wins(emu):
    ic.case_nearest_wins(emu)


def test_issue_independence(emu):
    ic.case_issue_independence(emu)


def test_long_list(emu):
    ic.case_long_list(emu)


def test_defaults_and_refusals(emu):
    ic.case_defaults_and_refusals(emu)


# ---- the checker must see a result that is slightly wrong: faults seeded into a copy of the RESULT, not into the kernel -------------

def _rejects(got, adm):
    with pytest.raises(AssertionError, match="outside the admissible set"):
        idref.check(got, adm, "seeded fault")


def test_checker_rejects_shifted_ids(emu):
    V, T, part, _ = ic.room(2000)
    cam, adm = ic.room_reference(2000, 160, 120, ic.ROOM_POSES[0])
    m = emu.mesh(V, T, part)
    ids, _, _ = emu.ids(m, cam)
    emu.free(m)
    idref.check(ids, adm, "unseeded")
    _rejects(np.roll(ids, 1, axis=1), adm)                                       # ids shifted one pixel
    _rejects(np.roll(ids, 1, axis=0), adm)


def test_checker_rejects_farther_label_and_painted_none(emu):
    cam = ic.quad_cam()
    Va, Ta = ic.quad(2.0, 0.4)
    Vb, Tb = ic.quad(3.0, 1.0)
    V, T, labels = np.concatenate([Va, Vb]), np.concatenate([Ta, Tb + 4]), [1, 1, 2, 2]
    adm = idref.admissible(V, T, labels, cam)
    m = emu.mesh(V, T, labels)
    ids, _, _ = emu.ids(m, cam)
    emu.free(m)
    idref.check(ids, adm, "unseeded")
    dec = adm["decided"].reshape(ids.shape)
    near = dec & (ids == 1)
    assert near.sum() > 200
    far = ids.copy()
    far[near] = 2                                                                # the farther surface's label
    _rejects(far, adm)
    one = ids.copy()
    y, x = np.argwhere(near)[near.sum() // 2]
    one[y, x] = 2                                                                # ... at a single pixel
    _rejects(one, adm)
    hole = ids.copy()
    hole[y, x] = idref.ID_NONE                                                   # -1 painted over a decided pixel
    _rejects(hole, adm)
    paint = ids.copy()
    y, x = np.argwhere(dec & (ids == idref.ID_NONE))[0]
    paint[y, x] = 2                                                              # and a label painted where nothing can be hit
    _rejects(paint, adm)
