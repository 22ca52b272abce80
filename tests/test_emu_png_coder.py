"""The deflate coder of the PNG encoder (csrc/sgs_png.h) where its code lengths hit their limits, under the wave64 emulator.

12 the reference of the coder checks itself (zlib's own Z_RLE streams parse to the reference's run parse; damaged streams are refused;
package-merge against the unconstrained optimum).  13 pictures built to reach the coder's branches (png_cases.coder_set): each one's
property is asserted from the reference alone, then the file goes through check_file, whose check_strip_coding holds every strip's
tokens, both codes and the stored / dynamic decision.  14 seeded faults that those checks must catch, each by the assertion named for
it.  15 padded frame strides, and batches of more than 256 strips.  Figures are printed (pytest -s) and listed in DESIGN.md §12."""
import re
import zlib

import numpy as np
import pytest

import emu_harness
import jpeg_cases
import png_cases as pc
import png_ref
from sage_gs import _capi


@pytest.fixture(scope="module")
def drv():
    d = pc.AbiPng(_capi.Lib(emu_harness.build_emu()))
    yield d
    d.close()


CODER = pc.coder_set()


# ---- 12: the reference ------------------------------------------------------------------------------------------------------------------
def _sample_strips():
    rs = np.random.RandomState(4)
    runs = np.repeat(rs.randint(0, 5, 400), rs.randint(1, 600, 400)).astype(np.uint8)[:16384].tobytes()
    return {"runs": runs, "text": (b"abcabcabd" * 300)[:2500], "aaaa": b"a" * 1000, "noise": rs.bytes(3000), "short": b"\x00\x00\x00", "one": b"\x07",
            "dyadic": pc.reference_strips(CODER["limit7_dyadic_2730x1"]["frame"], "rgb8")[1][0]}


def test_parser_reads_zlibs_rle_streams():
    """zlib's Z_RLE output (fixed, dynamic and stored blocks among them) parses to the reference's own run parse."""
    kinds = set()
    for name, strip in _sample_strips().items():
        blocks = png_ref.parse_deflate(png_ref.zlib_rle_stream(strip))
        kinds |= {b["type"] for b in blocks}
        assert [t for b in blocks for t in b["tokens"]] == png_ref.rle_tokens(strip), name
        assert blocks[-1]["type"] == 0 and blocks[-1]["tokens"] == [] and not blocks[-1]["final"]
    assert kinds == {0, 1, 2}
    whole = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    assert png_ref.parse_deflate(whole.compress(b"a" * 40) + whole.flush())[-1]["final"] == 1
    assert png_ref.rle_tokens(b"ab" + b"c" * 4 + b"d" * 3 + b"e" * 260 + b"f" * 262) == \
        [97, 98, 99, 256 + 3, 100, 100, 100, 101, 256 + 258, 101, 102, 256 + 258, 256 + 3]


def _bytes_of(bits):
    bits = bits + [0] * (-len(bits) % 8)
    return bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


def _dynamic_header(cl, hlit=257, hclen=19, body=()):
    """A dynamic block's first bits: BFINAL 0, BTYPE 2, HLIT, HDIST 1, HCLEN, the code-length code's lengths `cl` (by symbol)."""
    bits = [0, 0, 1]
    for v, n in ((hlit - 257, 5), (0, 5), (hclen - 4, 4)):
        bits += [(v >> k) & 1 for k in range(n)]
    for k in range(hclen):
        bits += [(cl[png_ref.CL_ORDER[k]] >> b) & 1 for b in range(3)]
    return _bytes_of(bits + list(body))


def test_deflate_parser_refuses_damage():
    """An over-subscribed and an incomplete code, a length over the limit, a repeat code with nothing before it, a code not in the
    table, a distance other than 1 or reaching before the strip, LEN != ~NLEN, a truncated stream."""
    def refused(stream, word):
        with pytest.raises(png_ref.PngError, match=word):
            png_ref.parse_deflate(stream)

    cl = [0] * 19
    cl[0] = cl[16] = 1
    refused(_dynamic_header(cl, body=[1]), "repeat code 16 with nothing before it")          # symbol 16 has code 1
    refused(_dynamic_header([1, 1, 1] + [0] * 16), "over-subscribed")
    refused(_dynamic_header([1, 2] + [0] * 17), "code of the code lengths: incomplete")
    with pytest.raises(png_ref.PngError, match="limit 7"):
        png_ref._decoder([8, 1], 7, "code of the code lengths")
    with pytest.raises(png_ref.PngError, match="limit 15"):
        png_ref._decoder([16, 1], 15, "literal / length code")
    with pytest.raises(png_ref.PngError, match="literal / length code: incomplete"):
        png_ref._decoder([1, 2], 15, "literal / length code")
    png_ref._decoder([1], 15, "distance code", may_be_partial=True)
    # an incomplete code cannot be stated in the stream's own terms without the parser refusing it first; "a code not in the table"
    # is what a partial distance code (one code of one bit: RFC 1951 allows it) leaves for the other bit
    table = png_ref._decoder([1], 15, "distance code", may_be_partial=True)
    with pytest.raises(png_ref.PngError, match="not in the table"):
        png_ref._symbol(png_ref._Bits(b"\xff\xff"), table, 15, "distance code")
    stored = bytes([0, 3, 0, 0xFC, 0xFF]) + b"abc" + bytes([0, 0, 0, 0xFF, 0xFF])
    assert [b["tokens"] for b in png_ref.parse_deflate(stored)] == [[97, 98, 99], []]
    refused(stored[:3] + b"\xfd" + stored[4:], "LEN")
    refused(stored[:-1], "ends inside")
    refused(bytes([0x06]), "reserved block type")
    # fixed-code blocks: "ab" + a match of 3 at distance 2; a match at distance 1 before any byte
    lit = lambda v: [((0x30 + v) >> k) & 1 for k in range(7, -1, -1)]
    match3 = [0, 0, 0, 0, 0, 0, 1]                          # symbol 257: 7 bits
    dist = lambda s: [(s >> k) & 1 for k in range(4, -1, -1)]
    eob = [0] * 7
    refused(_bytes_of([1, 1, 0] + lit(97) + lit(98) + match3 + dist(1) + eob), "distance 2")
    refused(_bytes_of([1, 1, 0] + match3 + dist(0) + eob), "reaches before the strip")
    ok = png_ref.parse_deflate(_bytes_of([1, 1, 0] + lit(97) + match3 + dist(0) + eob))
    assert ok[0]["tokens"] == [97, 256 + 3]
    # damage to zlib's own stream: a flipped bit in the table of a dynamic block
    strip = _sample_strips()["dyadic"]
    good = png_ref.zlib_rle_stream(strip)
    assert png_ref.parse_deflate(good)[0]["type"] == 2
    n_bad = 0
    for bit in range(17, 17 + 3 * 12):                      # the first twelve lengths of the code of the code lengths
        bad = bytearray(good); bad[bit >> 3] ^= 1 << (bit & 7)
        try:
            got = [t for b in png_ref.parse_deflate(bytes(bad)) for t in b["tokens"]]
            n_bad += got != png_ref.rle_tokens(strip)
        except png_ref.PngError:
            n_bad += 1
    assert n_bad == 36, "a flipped table bit went unnoticed"


def test_optimal_costs_of_the_reference():
    """package_merge equals the unconstrained optimum where that fits, exceeds it where it does not, and equals a brute force over
    all complete codes of five symbols; huffman_depths gives the optimal code of the least depth."""
    import itertools
    rs = np.random.RandomState(8)
    for _ in range(30):
        f = rs.randint(0, 50, 12).tolist()
        if sum(1 for x in f if x) < 2:
            continue
        d = png_ref.huffman_depths(f)
        best = png_ref.code_cost(f, [d.get(i, 0) for i in range(12)])
        assert png_ref.package_merge(f, max(d.values())) == best and png_ref.package_merge(f, 15) == best
        assert png_ref.kraft(d.values(), 15) == 1 << 15
    f = pc.strict_chain(8)
    assert max(png_ref.huffman_depths(f).values()) == 7
    for limit in (3, 4, 5, 6):
        brute = min(sum(a * b for a, b in zip(f, ls)) for ls in itertools.product(range(1, limit + 1), repeat=8) if png_ref.kraft(ls, limit) == 1 << limit)
        assert png_ref.package_merge(f, limit) == brute, (limit, brute)
        lim, steps = png_ref.limited_lengths(f, limit)
        assert steps > 0 and png_ref.kraft(lim.values(), limit) == 1 << limit and png_ref.code_cost(f, lim) >= brute
    assert max(png_ref.huffman_depths([1, 1, 2, 2]).values()) == 2          # {3, 3, 2, 1} costs the same and is deeper
    # no strip can be deeper than 18: the chain of 20 symbols that a depth of 19 needs weighs more than a strip has bytes
    assert sum(pc.strict_chain(20)) == 17710 > png_ref.STRIP and sum(pc.strict_chain(19)) == 10945


# ---- 13: the pictures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CODER))
def test_coder_pictures(drv, name):
    """The property from the reference alone, then checks 1-5 with the coder's own (2b) on the library's file."""
    case = CODER[name]
    want = pc.check_coder_case(name, case)                  # before the library's output is looked at
    h, w = case["frame"].shape[:2]
    fig = pc.check_file(drv.encode_one(case["frame"], case["fmt"]), pc.samples_of(case["frame"], case["fmt"]), drv.bound(w, h, case["fmt"]), name)
    want.pop("runs", None)
    print(f"[png coder] {name}: reference {want}; file {fig['coding']}")
    if "dynamic" in case["want"] or "depth15" in case["want"] or "depth7" in case["want"]:
        assert fig["coding"][0]["dynamic"]
    if "decision" in case["want"]:
        assert fig["coding"][0]["dynamic"] == (case["want"]["decision"] < 0)


def test_no_table_has_a_single_code_length_symbol():
    """`ncl < 2` in k_png_strips cannot be reached: the table always holds a non-zero length (the end of block's); if any of the 257
    symbols is unused it also holds a zero, and 257 used symbols cannot share one length (257 / 2^l is never 1), so two different
    lengths stand in it.  The reference counts at least two code-length symbols on every strip of every picture."""
    sets = [(f, "rgb8") for f in pc.colour_set().values()] + [(f, "depth16") for f in pc.depth_set().values()] + [(c["frame"], c["fmt"]) for c in CODER.values()]
    for frame, fmt in sets:
        for strip in pc.reference_strips(frame, fmt)[1]:
            assert sum(1 for f in png_ref.dynamic_block_model(png_ref.rle_tokens(strip))["cl_freq"] if f) >= 2


# ---- 14: seeded faults --------------------------------------------------------------------------------------------------------------------
H = "sgs_png.h"
SPLIT = "if (T >= 258u) { t0 = 256u + 258u; n = 1; T -= 258u; }"
SPLIT_AFTER = ("\n            if (T >= 3u) {", "\n            pending = T;")      # the line stands twice in the file: what follows each
MUTANTS = {          # name: {file of csrc/: [(anchor, replacement)]}
    "clamp_counts_at_limit_minus_1": {H: [("num[A[i] < (unsigned)limit ? A[i] : (unsigned)limit]++", "num[A[i] < (unsigned)limit - 1u ? A[i] : (unsigned)limit]++")]},
    "repair_splits_the_shallowest": {H: [("for (int i = limit - 1; i > 0; --i)\n            if (num[i]) {", "for (int i = 1; i < limit; ++i)\n            if (num[i]) {")]},
    "longest_to_the_most_frequent": {H: [("tab[sym[j++]] = (unsigned)len << 16;", "tab[sym[n - 1 - j++]] = (unsigned)len << 16;")]},
    "carry_dropped": {H: [("pending = T;", "pending = 0;")]},
    "split_at_257": {H: [(SPLIT + after, SPLIT.replace("258u", "257u") + after) for after in SPLIT_AFTER]},
    "filter_ties_to_the_highest": {H: [(f"if (s{k} < best)", f"if (s{k} <= best)") for k in (1, 2, 3, 4)]},
    "stored_only_when_longer": {H: [("if (len_dyn < len_stored) {", "if (len_dyn <= len_stored) {")]},
    "seven_bit_code_repaired": {H: [("s_cltab, 19, s_num, s_key);", "s_cltab, 19, s_num);")]},
    "hclen_not_trimmed": {H: [("while (hclen > 4 && !(s_cltab[order[hclen - 1]] >> 16)) --hclen;", "")]},
}
# `carry = 0;` before the second token pass is not among them: the carry is zero there anyway (the last window's lane 63 has no byte
# after it, so it never leaves a pending run), and a mutant without the line makes the same bytes.
CAUGHT_BY = {
    "clamp_counts_at_limit_minus_1": r"literal / length code: incomplete code",
    # (on a chain — and a code deeper than 15 in 16 384 tokens is nearly one — splitting the shallowest code moves every symbol below it
    # up a level and costs a byte, far under the cap on the excess over package-merge: the restated construction's size catches it)
    "repair_splits_the_shallowest": r"the dynamic coding takes 1392 bytes, the documented construction 1391",
    "longest_to_the_most_frequent": r"lengths increase with frequency",
    "carry_dropped": r"tokens differ from the run parse",
    "split_at_257": r"tokens differ from the run parse",
    "filter_ties_to_the_highest": r"filter types",
    "stored_only_when_longer": r"although not shorter than stored",
    "seven_bit_code_repaired": r"code of the code lengths: 477 symbol bits are 0.846 % over the optimal 7-bit code's 473",
    "hclen_not_trimmed": r"HCLEN 19 is not the smallest",
}


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """Every mutant's emulator library, compiled side by side (one g++ each)."""
    return emu_harness.build_mutants(tmp_path_factory.mktemp("png_mutants"), MUTANTS, "libsage_gs_png_mutant.so")


TIE = pc.colour_set()["filter_tie_48x32"]


def _coder_checks(d):
    """check_file (with check_strip_coding) on the coder's pictures and on the picture of tied filters."""
    for name, case in sorted(CODER.items(), key=lambda kv: not kv[0].startswith("three_symbols")):       # (the strip that stays dynamic under any code first)
        h, w = case["frame"].shape[:2]
        pc.check_file(d.encode_one(case["frame"], case["fmt"]), pc.samples_of(case["frame"], case["fmt"]), d.bound(w, h, case["fmt"]), name)
    pc.check_file(d.encode_one(TIE, "rgb8"), png_ref.rgb_samples(TIE), d.bound(48, 32, "rgb8"), "filter_tie_48x32")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_png_mutant_is_caught(mutant_libs, name):
    d = pc.AbiPng(_capi.Lib(mutant_libs[name]))
    caught = None
    try:
        _coder_checks(d)
    except (AssertionError, png_ref.PngError) as e:
        caught = e
    finally:
        d.close()
    assert caught is not None, f"{name}: the coder's checks pass on this mutant"
    assert re.search(CAUGHT_BY[name], f"{type(caught).__name__}: {caught}"), f"{name}: failed on another assertion: {str(caught)[:300]}"
    print(f"[png mutant] {name}: caught: {str(caught)[:200]}")


def test_the_unmutated_library_passes_the_mutants_checks(drv):
    _coder_checks(drv)


# ---- 15: padded strides, long scans ---------------------------------------------------------------------------------------------------------
def test_padded_stride_and_long_scan(drv):
    """Frames a frame plus 37 floats apart (NaN and 1e30 between them) give the packed batch's files; a batch of 258 strips has the
    offsets and sizes of its files end to end, writes nothing beyond them, and gives every frame the bytes it gets alone.  Colour (two
    strips a frame) and depth (one strip a frame, 257 frames)."""
    frames = pc.long_scan_frames()
    batch = jpeg_cases.check_stride_and_long_scan(drv.encode, frames, 256, 2, fmt="rgb8")
    assert len(set(batch["files"])) == len(frames)
    for i in (0, 1, 63, 64, 127, 128):
        assert drv.encode_one(frames[i], "rgb8") == batch["files"][i], f"frame {i} depends on the batch it is issued in"
    depth = np.stack([pc.depth_levels(9, 5) * np.float32(1 + 0.01 * i) for i in range(257)])
    dbatch = jpeg_cases.check_stride_and_long_scan(drv.encode, depth, 256, 1, fmt="depth16")
    for i in (0, 128, 255, 256):
        assert drv.encode_one(depth[i], "depth16") == dbatch["files"][i]
    pc.check_file(batch["files"][128], png_ref.rgb_samples(frames[128]), drv.bound(2731, 2, "rgb8"), "long_scan_frame_128")
