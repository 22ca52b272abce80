"""The emulator harness itself (tests/emu_harness.py): which files make a library stale, when, and how a copy of csrc/ is edited.
Nothing here compiles."""
import os

import pytest

import emu_harness

CSRC = os.path.join(emu_harness.PKG, "csrc")


def test_the_source_list_is_the_directory():
    listed = sorted(os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith(".h") or n.endswith(".hip"))
    outside = [os.path.join(emu_harness.EMU_DIR, "hip", "hip_runtime.h"), os.path.join(emu_harness.ROOT, "include", "sage_gs.h")]
    assert sorted(emu_harness.sources()) == sorted(listed + outside) and all(os.path.isfile(p) for p in outside)
    names = {os.path.basename(p) for p in emu_harness.sources()}
    assert {"sgs_api.hip", "sgs_similarity.h", "sgs_topdown.h", "sgs_clearance.h", "sgs_geodesic.h"} <= names


def test_a_copy_of_csrc_is_listed_the_same_way(tmp_path):
    for n in ("a.h", "b.hip", "notes.txt", "c.h.orig"):
        (tmp_path / n).write_text("")
    assert emu_harness.sources(tmp_path) == [str(tmp_path / "a.h"), str(tmp_path / "b.hip")] + emu_harness.sources()[-2:]


def test_stale(tmp_path):
    lib = tmp_path / "lib.so"
    srcs = [tmp_path / n for n in ("a.h", "b.h", "c.hip")]
    for p in [lib] + srcs:
        p.write_text("")
    for p in srcs:
        os.utime(p, (1000, 1000))
    os.utime(lib, (2000, 2000))
    assert not emu_harness.stale(str(lib), [str(p) for p in srcs])                   # the library is newest
    for p in srcs:                                                                   # any one file newer than it
        os.utime(p, (3000, 3000))
        assert emu_harness.stale(str(lib), [str(q) for q in srcs]), p.name
        os.utime(p, (1000, 1000))
    assert not emu_harness.stale(str(lib), [str(p) for p in srcs])
    lib.unlink()
    assert emu_harness.stale(str(lib), [str(p) for p in srcs])                       # no library


def test_edits_need_every_anchor_exactly_once_and_apply_in_order(tmp_path):
    text = "#define A 1\n#define B 2\n#define B 2\n"
    hdr = tmp_path / "small.h"
    hdr.write_text(text)
    with pytest.raises(AssertionError, match=r"small\.h: anchor found 0 times: '#define C'"):
        emu_harness.apply_edits(tmp_path, {"small.h": [("#define C", "")]})
    with pytest.raises(AssertionError, match=r"small\.h: anchor found 2 times: '#define B 2\\n'"):
        emu_harness.apply_edits(tmp_path, {"small.h": [("#define B 2\n", "")]})
    assert hdr.read_text() == text                                                   # a refused edit leaves the file alone
    # the second anchor lies inside the first replacement; the third occurs once only after the second was applied
    emu_harness.apply_edits(tmp_path, {"small.h": [("#define A 1", "#define A (X + 1)"), ("X + 1", "7"), ("#define B 2\n#define B 2\n", "#define B 2\n"),
                                                   ("#define B 2\n", "")]})
    assert hdr.read_text() == "#define A (7)\n"
