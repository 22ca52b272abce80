"""The PNG encoder's checks, shared by the CPU-emulator tests (test_emu_png.py) and the GPU tests (test_gpu_png.py): the picture set, a
driver of the C ABI over plain buffers, and the assertions on a file (lossless, structure, filters, the deflate coder strip by strip,
sizes, against zlib on the same strips); pictures built to reach the coder's branches, each with its property (coder_set)."""
from __future__ import annotations

import ctypes as C
import io
import zlib

import numpy as np

import jpeg_cases
import png_ref
from abi_driver import SENTINEL, GpuBuffers  # noqa: F401  (SENTINEL: the tests name it as png_cases.SENTINEL)

# Test 5: our file against zlib restricted to the same design (the same filtered bytes, every strip deflated alone at level 1 with run
# matches only, the same framing).  The worst ratio over the whole picture set, measured on the emulator build (whose bytes are the
# GPU's), was 1.0519 (depth_1x1: 81 bytes against 77, and colour_1x1: 82 against 78 — a strip of 3 or 4 bytes, which we store and zlib
# puts into a fixed-code block; every picture of more than a few hundred bytes is within 0.01 % of zlib or below it); rounded up to the
# next whole per cent plus two points.  DESIGN.md §12 and profiles/png_sizes_emulator.json hold the table.
RLE_MARGIN = 1.08
# Check 4's "smaller than raw" cannot hold for a picture of a few hundred bytes: a PNG file has 57 bytes of framing before its first
# sample and a dynamic block some 60-100 bytes of code lengths.  Pictures under this many raw bytes are held to sgs_png_bound alone.
SMALLER_THAN_RAW_FROM = 4096


def colour_set():
    """name -> fp32 [H,W,3]."""
    g = jpeg_cases.gradient_noise
    rs = np.random.RandomState(11)
    period = np.float32([[0.1, 0.5, 0.9], [0.7, 0.2, 0.4], [0.3, 0.8, 0.6]])
    yy, xx = np.mgrid[0:40, 0:96]
    tie = np.zeros((32, 48, 3), np.float32)                # rows of zeros: all five filters tie; equal rows below: Up ties with Paeth
    tie[8:16] = 0.4
    tie[16:24] = g(8, 48, 2)[0:1]
    tie[24:] = g(8, 48, 3)
    return {
        "colour_1x1": g(1, 1, 1), "colour_7x5": g(5, 7, 7), "colour_17x33": g(33, 17, 4), "colour_250x187": g(187, 250, 6),
        "colour_256x192": g(192, 256, 5),
        "colour_2730x3": g(3, 2730, 8),                    # rows of 8 191 filtered bytes: two fit a strip, the third does not
        "colour_5461x2": g(2, 5461, 9),                    # the longest legal row: one-row strips
        "constant_640x48": np.broadcast_to(np.float32([0.3, 0.6, 0.9]), (48, 640, 3)).copy(),
        "noise_64x64": rs.rand(64, 64, 3).astype(np.float32),
        "all_255_64x32": np.ones((32, 64, 3), np.float32),
        "period3_96x40": period[(xx + yy) % 3].astype(np.float32),
        "out_of_range_33x17": jpeg_cases.out_of_range(),
        "filter_tie_48x32": tie,
    }


def analytic_room(w=160, h=120):
    """Distance to the image plane of the walls of a 4 x 3 x 6 m box seen from inside (camera yawed and pitched, so every plane is
    oblique), with patches of +inf, -inf, NaN, negative values and values beyond 6.5 m."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 0.6 * w
    d = np.stack([(xx - w / 2 + 0.5) / f, (yy - h / 2 + 0.5) / f, np.ones_like(xx)], -1)
    cy, sy, cp, sp = np.cos(0.5), np.sin(0.5), np.cos(0.2), np.sin(0.2)
    rot = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    dw = d @ rot.T
    o = np.array([0.3, -0.2, -0.5]); half = np.array([2.0, 1.5, 3.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dw > 0, (half - o) / dw, np.where(dw < 0, (-half - o) / dw, np.inf)).min(-1)
    depth = t.astype(np.float32)                           # the ray's camera-space z is 1: t is the distance to the image plane
    depth[5:15, 10:30] = np.inf; depth[20:30, 40:50] = -np.inf; depth[40:44, 5:60] = np.nan
    depth[60:70, 100:130] = -1.25; depth[80:100, 20:60] += 5.0; depth[110:, 150:] = 1.0e9
    return depth


def depth_levels(w=37, h=21):
    """Values exactly on k / 10000 (a ramp of k, as far as fp32 can hold them) and their fp32 neighbours above and below."""
    yy, xx = np.mgrid[0:h, 0:w]
    k = (xx * 37 + yy * 53 + 11).astype(np.float32)
    d = k / np.float32(10000.0)
    d[::3] = np.nextafter(d[::3], np.float32(10.0))
    d[1::3] = np.nextafter(d[1::3], np.float32(-10.0))
    return d


def depth_set():
    """name -> fp32 [H,W]."""
    return {
        "depth_room_160x120": analytic_room(),
        "depth_levels_37x21": depth_levels(),
        "depth_1x1": np.float32([[1.2345]]),
        "depth_8191x1": np.linspace(0.5, 6.0, 8191, dtype=np.float32)[None, :],
    }


def samples_of(frame, fmt, depth_scale=10000.0, depth_max=6.5):
    return png_ref.rgb_samples(frame) if fmt == "rgb8" else png_ref.depth_samples(frame, depth_scale, depth_max)


class AbiPng(jpeg_cases.AbiEncoder):
    """sgs_encode_png: frames fp32 [n,H,W,3] (rgb8) or [n,H,W] (depth16); encode(frames, fmt, depth_scale=, depth_max=, ...)."""
    ENCODE, STATUS = "sgs_encode_png", "sgs_png_status"

    def _params(self, fmt="rgb8", depth_scale=10000.0, depth_max=6.5):
        return self._capi.png_params(fmt, depth_scale, depth_max)

    def bound(self, w, h, fmt="rgb8", depth_scale=10000.0, depth_max=6.5):
        return int(self.lib.sgs_png_bound(int(w), int(h), C.byref(self._params(fmt, depth_scale, depth_max))))


class GpuPng(GpuBuffers, AbiPng):
    """AbiPng over torch device buffers, on a Renderer's context."""


def pil_size(samples, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(samples).save(b, "PNG", **kw)
    return len(b.getvalue())


def check_file(data, samples, bound, label="", against_zlib=True):
    """Checks 1-5 (and 2b, the coder: check_strip_coding) on one file against the samples it must hold (uint8 [H,W,3] or uint16
    [H,W]); prints and returns the figures.
    against_zlib=False prints check 5's ratio without asserting it (for rows of ten samples beside the picture set, which test sample
    values: a strip of 21 bytes is stored behind 10 bytes of block framing, and zlib's fixed-code block has none)."""
    from PIL import Image
    samples = np.ascontiguousarray(samples)
    raw, bpp = png_ref.raw_rows(samples)
    h, nb = raw.shape
    w = nb // bpp
    # 2 structure
    parsed = png_ref.parse_png(data)                        # signature, every CRC, nothing after IEND
    rps = png_ref.strip_rows(nb + 1)
    n_strips = -(-h // rps)
    names = [t for t, _ in parsed["chunks"]]
    assert names == [b"IHDR"] + [b"IDAT"] * n_strips + [b"IEND"], (label, names[:4], len(names), n_strips)
    assert parsed["ihdr"] == (w, h, 8 if bpp == 3 else 16, 2 if bpp == 3 else 0, 0, 0, 0), parsed["ihdr"]
    assert parsed["chunks"][-1][1] == b""
    idat = [b for t, b in parsed["chunks"] if t == b"IDAT"]
    streams = strip_streams(parsed, n_strips)
    blocks = [png_ref.parse_deflate(st) for st in streams]  # every code complete and within its limit, every block well-formed (PngError)
    # 2b the coder, read by the reference alone (a fault is named here, before zlib and PIL meet it): the filter types where the rows
    # have their length, then the tokens, both codes and the stored / dynamic decision of every strip
    types, filtered, tied = png_ref.filter_rows(raw, bpp)
    own = b"".join(png_ref.expand_tokens(t) for bl in blocks for b in bl for t in [b["tokens"]])
    if len(own) == h * (nb + 1):
        own_types = list(own[::nb + 1])
        assert own_types == types, f"{label}: filter types {own_types[:12]}.. expected {types[:12]}.."
    coding = check_strip_coding(streams, [filtered[y:y + rps].tobytes() for y in range(0, h, rps)], label, blocks)
    # 1 lossless
    im = Image.open(io.BytesIO(data)); im.load()
    assert im.mode == ("RGB" if bpp == 3 else "I;16") and im.size == (w, h), (im.mode, im.size)
    assert np.array_equal(np.asarray(im), samples), f"{label}: PIL reads other samples"
    z = zlib.decompressobj()
    inflated = z.decompress(b"".join(idat)) + z.flush()
    assert z.eof and z.unused_data == b"" and len(inflated) == h * (nb + 1), (label, z.eof, len(z.unused_data), len(inflated))
    assert idat[0][:2] == b"\x78\x01"
    # 3 filters (and, with them, every filtered byte)
    got = np.frombuffer(inflated, np.uint8).reshape(h, nb + 1)
    assert got[:, 0].tolist() == types, f"{label}: filter types {got[:, 0].tolist()[:12]}.. expected {types[:12]}.."
    assert np.array_equal(got, filtered), f"{label}: filtered bytes differ"
    # 2, last item: every strip inflates alone as a raw deflate stream to its own rows, and ends on the empty stored block
    for s, body in enumerate(idat):
        part = body[2 if s == 0 else 0:len(body) - (9 if s == n_strips - 1 else 0)]
        d = zlib.decompressobj(-15)
        rows = d.decompress(part)
        want = filtered[s * rps:(s + 1) * rps].tobytes()
        assert rows == want and d.unused_data == b"" and d.unconsumed_tail == b"" and not d.eof, f"{label}: strip {s} does not stand alone"
        assert part[-4:] == b"\x00\x00\xff\xff", f"{label}: strip {s} does not end on an empty stored block"
    assert idat[-1][-9:-4] == b"\x01\x00\x00\xff\xff"
    # 4 sizes
    raw_bytes = h * nb
    assert len(data) <= bound, (label, len(data), bound)
    # 5 against zlib on the same strips, run matches only
    ref = png_ref.zlib_rle_file_size(filtered, n_strips, rps)
    pil1, pild = pil_size(samples, compress_level=1), pil_size(samples)
    ratio = len(data) / ref
    print(f"[png] {label} {w}x{h}: {len(data)} bytes, raw {raw_bytes}, bound {bound}, zlib level 1 Z_RLE on the same strips {ref} (x{ratio:.4f}), "
          f"PIL compress_level=1 {pil1} (x{len(data) / pil1:.3f}), PIL default {pild} (x{len(data) / pild:.3f}), {n_strips} strips, "
          f"filters used {sorted(set(types))}, rows with tied filters {sum(tied)}")
    assert not against_zlib or ratio <= RLE_MARGIN, f"{label}: {len(data)} bytes is {ratio:.4f} x zlib's {ref} on the same strips (allowed {RLE_MARGIN})"
    return {"bytes": len(data), "raw": raw_bytes, "bound": bound, "zlib_rle_same_strips": ref, "ratio_to_zlib_rle": round(ratio, 4),
            "pil_level1": pil1, "pil_default": pild, "strips": n_strips, "tied_rows": int(sum(tied)), "coding": coding}


def check_smaller_than_raw(fig, label, noise=False):
    """Check 4's last item: every picture but noise is smaller than its raw bytes (from SMALLER_THAN_RAW_FROM raw bytes on)."""
    if not noise and fig["raw"] >= SMALLER_THAN_RAW_FROM:
        assert fig["bytes"] < fig["raw"], f"{label}: {fig['bytes']} bytes, raw {fig['raw']}"


# ---- the deflate coder: what every strip's block must be (check_strip_coding), and pictures built to reach its branches ----------------
# Where the optimal code is deeper than the limit, the construction (fold to the limit, repair the Kraft sum) is a heuristic: its
# symbol bits are held to package-merge's optimal length-limited cost plus this share.  Measured over coder_set() on the emulator
# build (DESIGN.md §12 has the table): worst excess at 15 bits 0.0141 % (limit15_depth18_full), at 7 bits 0 (limit7_dyadic_2730x1: one repair step, and
# the optimal 7-bit code costs the same); each cap is that figure
# rounded up to the next tenth of a per cent plus one tenth (the bytes are deterministic: the margin is room for re-seeding a case).
EXCESS_CAP_15 = 0.002
EXCESS_CAP_7 = 0.001


def strip_streams(parsed, n_strips):
    """The raw deflate stream of every strip's IDAT chunk: without the zlib header of the first and the final block + Adler-32 of
    the last."""
    idat = [b for t, b in parsed["chunks"] if t == b"IDAT"]
    return [body[2 if s == 0 else 0:len(body) - (9 if s == n_strips - 1 else 0)] for s, body in enumerate(idat)]


def _never_increase(freq, lengths, what, label):
    by = sorted((f, lengths[s]) for s, f in enumerate(freq) if f)
    longest_above = 0
    for k in range(len(by) - 1, -1, -1):                   # from the most frequent down: no rarer symbol may be shorter
        f, l = by[k]
        tail = [x[1] for x in by[k + 1:] if x[0] > f]
        longest_above = max(tail) if tail else 0
        assert l >= longest_above, f"{label}: {what}: lengths increase with frequency (a symbol seen {f} times has {l} bits, a more frequent one {longest_above})"


def _held_to_optimum(freq, lengths, limit, cap, what, label):
    """Symbol bits against the optimal code (exactly, where it fits the limit) or against package-merge (within the cap)."""
    depth = max(png_ref.huffman_depths(freq).values())
    bits = png_ref.code_cost(freq, lengths)
    if depth <= limit:
        best = png_ref.code_cost(freq, png_ref.huffman_depths(freq))
        assert bits == best, f"{label}: {what}: {bits} symbol bits, the optimal code takes {best}"
        return depth, 0.0
    best = png_ref.package_merge(freq, limit)
    excess = bits / best - 1.0
    assert bits >= best, f"{label}: {what}: {bits} symbol bits are fewer than the optimal {limit}-bit code's {best}: the reference is wrong"
    assert excess <= cap, f"{label}: {what}: {bits} symbol bits are {100 * excess:.3f} % over the optimal {limit}-bit code's {best} (cap {100 * cap:.1f} %)"
    return depth, excess


def check_strip_coding(streams, strips, label="", parsed_blocks=None):
    """Every strip's deflate stream (strip_streams) against the reference's filtered bytes of the strip: the block structure, the
    stored / dynamic decision, the tokens, both codes (complete, within 15 / 7 bits, lengths never increasing with frequency, HLIT and
    HCLEN the smallest, the run-length coded table as documented, the symbol bits optimal or within the cap of package-merge).  Returns
    one dict of figures per strip."""
    figs = []
    for s, (part, want) in enumerate(zip(streams, strips)):
        lab = f"{label} strip {s}"
        blocks = png_ref.parse_deflate(part) if parsed_blocks is None else parsed_blocks[s]      # PngError on any malformed code or block
        assert len(blocks) == 2 and not blocks[0]["final"], f"{lab}: {len(blocks)} blocks (one and the empty stored block expected)"
        assert blocks[1]["type"] == 0 and blocks[1]["tokens"] == [] and not blocks[1]["final"], f"{lab}: the last block is not an empty stored block"
        main = blocks[0]
        tokens = png_ref.rle_tokens(want)
        dyn, stored = png_ref.strip_chunk_sizes(tokens, len(want))
        fig = {"bytes": len(want), "dynamic": main["type"] == 2, "dynamic_bytes": dyn, "stored_bytes": stored}
        figs.append(fig)
        if main["type"] == 0:
            assert dyn >= stored, f"{lab}: stored ({stored} bytes) although the dynamic block is shorter ({dyn})"
            assert bytes(main["data"]) == bytes(want) and len(part) == stored, f"{lab}: the stored block does not hold the strip"
            continue
        assert main["type"] == 2, f"{lab}: block type {main['type']}"
        assert len(part) < stored, f"{lab}: dynamic ({len(part)} bytes) although not shorter than stored ({stored})"
        assert main["tokens"] == tokens, f"{lab}: the tokens differ from the run parse of the reference's filtered bytes (first at {next((i for i, (a, b) in enumerate(zip(main['tokens'], tokens)) if a != b), min(len(tokens), len(main['tokens'])))}: {len(main['tokens'])} tokens, reference {len(tokens)})"
        # the literal / length code
        freq, _ = png_ref.token_histogram(tokens)
        lit = main["litlen_lengths"] + [0] * (286 - main["hlit"])
        assert main["hdist"] == 1 and main["dist_lengths"] == [1], f"{lab}: distance code {main['dist_lengths']}"
        assert all((f > 0) == (l > 0) for f, l in zip(freq, lit)), f"{lab}: a used symbol without a code, or a code for an unused symbol"
        assert max(lit) <= 15 and png_ref.kraft(lit, 15) == 1 << 15, f"{lab}: literal / length code: Kraft sum {png_ref.kraft(lit, 15)} / 32768"
        _never_increase(freq, lit, "literal / length code", lab)
        assert main["hlit"] == max(257, max(i for i, f in enumerate(freq) if f) + 1), f"{lab}: HLIT {main['hlit']} is not the smallest that holds the used symbols"
        fig["depth15"], fig["excess15"] = _held_to_optimum(freq, lit, 15, EXCESS_CAP_15, "literal / length code", lab)
        # the code of the code lengths
        syms = [t[0] for t in png_ref.length_sequence_symbols(main["litlen_lengths"] + main["dist_lengths"])]
        assert main["cl_symbols"] == syms, f"{lab}: the code lengths are not run-length coded as documented"
        cl_freq = [syms.count(k) for k in range(19)]
        cl = main["cl_lengths"]
        assert sum(1 for f in cl_freq if f) >= 2, f"{lab}: one code-length symbol"      # (cannot happen: see coder_set)
        assert all((f > 0) == (l > 0) for f, l in zip(cl_freq, cl)), f"{lab}: code of the code lengths: a used symbol without a code, or a code for an unused one"
        assert max(cl) <= 7 and png_ref.kraft(cl, 7) == 1 << 7, f"{lab}: code of the code lengths: Kraft sum {png_ref.kraft(cl, 7)} / 128"
        _never_increase(cl_freq, cl, "code of the code lengths", lab)
        want_hclen = max(4, max(k for k in range(19) if cl[png_ref.CL_ORDER[k]]) + 1)
        assert main["hclen"] == want_hclen, f"{lab}: HCLEN {main['hclen']} is not the smallest that holds the used symbols ({want_hclen})"
        fig["depth7"], fig["excess7"] = _held_to_optimum(cl_freq, cl, 7, EXCESS_CAP_7, "code of the code lengths", lab)
        assert len(part) == dyn, f"{lab}: the dynamic coding takes {len(part)} bytes, the documented construction {dyn}"
    return figs


def ordered_without_repeats(counts, seed, first_not=0):
    """The values of {value: count} in a seeded random order in which no value follows itself and the first is not `first_not`."""
    rs = np.random.RandomState(seed)
    vals = sorted(counts)
    left = np.array([counts[v] for v in vals], np.int64)
    out, prev = [], vals.index(first_not) if first_not in counts else -1
    total = int(left.sum())
    for _ in range(total):
        w = left.astype(np.float64)
        if prev >= 0:
            w[prev] = 0
        k = int(np.argmax(left))
        if 2 * left[k] <= left.sum() or k == prev:          # the most frequent value must go now when it is half of what is left
            assert w.sum() > 0, "no order without repeats"
            k = int(np.searchsorted(np.cumsum(w), rs.rand() * w.sum(), side="right"))
        out.append(vals[k]); left[k] -= 1; prev = k
    return out


def strict_chain(n, start=(1, 1)):
    """n weights, ascending, whose optimal code is a chain of depth n - 1 whatever the tie rule: every weight exceeds the sum of all
    weights two and more places below it (Fibonacci's growth, the slowest that does it)."""
    w = list(start)
    while len(w) < n:
        w.append(max(w[-1], sum(w[:-1]) + 1))
    return w


def signed_values(n):
    """n byte values of the least magnitudes read as signed, none zero: 1, 255, 2, 254, ..."""
    return [(k // 2 + 1) if k % 2 == 0 else 256 - (k // 2 + 1) for k in range(n)]


def rgb_rows(raw_bytes, height=1):
    """fp32 [H, W, 3] on the levels k / 255 whose raw rows are the given bytes."""
    b = np.asarray(raw_bytes, np.uint8).reshape(height, -1, 3)
    frame = b.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(png_ref.rgb_samples(frame), b)
    return frame


def depth_rows(raw_bytes, height=1):
    """fp32 [H, W] in the middle of the levels, (k + 1/2) / 10000, whose raw rows are the given bytes (big-endian 16-bit samples)."""
    b = np.asarray(raw_bytes, np.uint8).reshape(height, -1, 2).astype(np.uint32)
    k = (b[..., 0] << 8) | b[..., 1]
    assert k.max() <= 64999
    frame = ((k.astype(np.float64) + 0.5) / 10000.0).astype(np.float32)
    assert np.array_equal(png_ref.depth_samples(frame), k.astype(np.uint16))
    return frame


def _chain_row(n_values, seed, runs=(), top_up_to=None):
    """One RGB row whose literal histogram is a strict chain: end of block 1, the filter byte 1, then n_values byte values (and, for
    `runs` = ((T, count), ...), the length symbols of `count` runs of T repeats each, which take the chain's lowest places)."""
    w = strict_chain(2 + len(runs) + n_values)
    for (T, count), have in zip(runs, w[2:]):
        assert count == have, (T, count, have)
    counts = dict(zip(reversed(signed_values(n_values)), w[2 + len(runs):]))        # the most frequent values nearest to zero
    top = max(counts, key=counts.get)
    extra = sum(T * c for T, c in runs)
    second = sorted(counts, key=counts.get)[-2]            # topping up the two most frequent values keeps the chain; an order without
    while (sum(counts.values()) + extra) % 3 or (top_up_to and sum(counts.values()) + extra + 3 <= top_up_to):      # repeats needs the top under half
        counts[second if top_up_to and 2 * counts[top] + 2 > top_up_to else top] += 1
    seq = ordered_without_repeats(counts, seed)
    at = [i for i, v in enumerate(seq) if v == top]
    rs = np.random.RandomState(seed + 1)
    where = {}
    for T, count in runs:
        for _ in range(count):
            where[at.pop(int(rs.randint(len(at))))] = T
    out = []
    for i, v in enumerate(seq):
        out.extend([v] * (1 + where.get(i, 0)))
    return rgb_rows(out)


# the runs picture: repeat counts T, each ending on these lanes of a 64-byte window
RUN_T = (1, 2, 3, 4, 257, 258, 259, 260, 261, 515, 516, 517, 519)
RUN_LANES = (0, 1, 62, 63)


def _runs_picture(width=2730, rows_per_strip=2):
    """RGB rows of zeros runs between fillers 1, 255, 1, ... (the None filter wins: everything is of magnitude <= 1 and no neighbour
    predicts it better): every T of RUN_T ending on every lane of RUN_LANES; a run whose 258th repeat falls on lane 63 while it goes
    on; a run across a row's filter byte; a run to the strip's last byte that goes on in the next strip."""
    rowlen = 3 * width + 1
    S = rows_per_strip * rowlen
    wanted = [(T, lane) for T in RUN_T for lane in RUN_LANES]
    strips, cur, c = [], None, 0

    def new_strip():
        nonlocal cur, c
        cur = np.array([1 if p % 2 else 255 for p in range(S)], np.uint8)
        cur[::rowlen] = 0
        strips.append(cur); c = 1

    def place(T, lane=None, start=None):
        """Zeros at [s, s + T] (the run's first byte and its T repeats) behind at least one filler byte; False if the strip is full."""
        nonlocal c
        s = c + 1 if start is None else start
        while True:
            if lane is not None and (s + T) % 64 != lane:
                s += 1; continue
            if (s - 1) % rowlen == 0 or (s + T + 1) % rowlen == 0:      # a filter byte would lengthen the run
                s += 1 if lane is None else 64; continue
            break
        if s + T + 2 > S:
            return False
        cur[s:s + T + 1] = 0
        c = s + T + 1
        return True

    new_strip()
    assert place(600, start=rowlen - 300)                  # across the filter byte of the strip's second row
    c = 1
    todo = list(wanted) + [(519, (61 + 519) % 64), (258 + 64, (61 + 258 + 64) % 64)]      # these start on lane 61: repeat 258 on lane 63
    for T, lane in todo:
        if rowlen - 300 - (T + 70) < c < rowlen + 301:      # jump the run placed first
            c = rowlen + 301
        if not place(T, lane):
            cur[S - 40:] = 0                                # a run to the strip's last byte, going on in the next strip
            new_strip()
            cur[1:30] = 0; c = 30
            assert place(T, lane)
    cur[S - 5:] = 0
    new_strip()                                            # the last strip starts inside a run again and ends on one of 2 repeats
    cur[1:4] = 0
    cur[S - 3:] = 0
    raw = np.concatenate([s.reshape(rows_per_strip, rowlen)[:, 1:].reshape(-1) for s in strips])
    return rgb_rows(raw, rows_per_strip * len(strips))


def _dyadic_row(seed=3):
    """One RGB row of 2730 pixels whose 8192 tokens (the filter byte and the end of block among them) have power-of-two frequencies,
    so that the literal lengths are dictated: 3 values of 2 bits, 1 of 3, 7 of 6, 1 of 7, 1 of 8, 3 of 12, 26 of 13.  The 42 used symbols
    lie apart by 1 zero (4 times), 2 zeros (4), 3 zeros (32) and once by 107: the run-length coded table has the histogram
    0: 12, 1: 1, 2: 3, 3: 1, 6: 7, 7: 1, 8: 1, 12: 3, 13: 26, 17: 32, 18: 1 — found by a random search over Kraft-complete tables for
    one whose code-length code is 8 deep."""
    gaps_low = [1, 1, 2, 2] + [3] * 16
    gaps_high = [1, 1, 2, 2] + [3] * 16
    low, high = [0], [256]
    for g in gaps_low:
        low.append(low[-1] + g + 1)
    for g in gaps_high:
        high.append(high[-1] - g - 1)
    used = low + high[::-1]
    assert len(used) == 42 and len(set(used)) == 42 and 11 <= high[-1] - low[-1] - 1 <= 138
    lengths = [2] * 3 + [3] + [6] * 7 + [7, 8] + [12] * 3 + [13] * 24
    values = sorted((v for v in used if v not in (0, 256)), key=lambda v: (min(v, 256 - v), v))     # the most frequent nearest to zero
    counts = {v: 1 << (13 - l) for v, l in zip(values, lengths)}
    return rgb_rows(ordered_without_repeats(counts, seed))


def _boundary_row(width, k, seed):
    """One RGB row of bytes drawn from k values: near the stored / dynamic decision for the right (width, k)."""
    rs = np.random.RandomState(seed)
    return rgb_rows(rs.randint(0, k, 3 * width).astype(np.uint8))


# name -> (width, k, seed, dynamic bytes - stored bytes by the reference's count): the first hits of a search over widths 60..200, k
# 20..256 and seeds 0..5 for the distances -1, 0 and +1 — the decision itself and its two neighbours
BOUNDARY = {"decision_dynamic_by_1_60x1": (60, 88, 1, -1), "decision_equal_60x1": (60, 72, 3, 0), "decision_stored_by_1_60x1": (60, 92, 3, 1)}


def coder_set():
    """name -> dict(fmt, frame, want): pictures of one strip or a few, built to reach the coder's branches.  `want` is the property
    check_coder_case asserts from png_ref alone."""
    zero = np.zeros((1, 1), np.float32)
    cases = {
        "limit15_depth15": dict(fmt="rgb8", frame=_chain_row(14, 21), want=dict(depth15=(15, 15))),
        "limit15_depth16": dict(fmt="rgb8", frame=_chain_row(15, 22), want=dict(depth15=(16, 16))),
        # 18 is the deepest a strip can reach: a code of depth 19 needs the weights of a chain of 20 symbols, at least 1 + 1 + 2 + 3 +
        # 5 + ... = 17 710 tokens, and a strip has at most 16 384 bytes
        "limit15_depth18_full": dict(fmt="rgb8", frame=_chain_row(17, 23, top_up_to=16383), want=dict(depth15=(18, 18), bytes=16384)),
        "limit15_lengths_deepest": dict(fmt="rgb8", frame=_chain_row(14, 24, runs=((3, 2), (4, 3))), want=dict(depth15=(17, 17), deepest=(256, 257))),
        "limit7_dyadic_2730x1": dict(fmt="rgb8", frame=_dyadic_row(), want=dict(depth7=(8, 8))),
        # the first hit of a search over rows of random bytes (widths 80..500, 8..200 values, seeds 0..7) whose code-length code is over 7
        # deep and on which folding and repairing (what the coder once did at 7 bits too) costs most: 477 bits against the optimal 473
        "limit7_repair_costs_500x1": dict(fmt="rgb8", frame=_boundary_row(500, 104, 3), want=dict(depth7=(8, 19), repair7_excess=4)),
        "two_symbols_depth_1x1": dict(fmt="depth16", frame=zero, want=dict(used=2)),
        "three_symbols_depth_8127x1": dict(fmt="depth16", frame=np.zeros((1, 8127), np.float32), want=dict(used=3, dynamic=True)),      # 0, 63 x 258, end
        "runs_2730x6": dict(fmt="rgb8", frame=_runs_picture(), want=dict(runs=True)),
    }
    for name, (w, k, seed, d) in BOUNDARY.items():
        cases[name] = dict(fmt="rgb8", frame=_boundary_row(w, k, seed), want=dict(decision=d))
    return cases


def long_scan_frames(n=129):
    """n different colour frames of 2731x2: rows of 8 194 filtered bytes, one per strip — 258 strips, so that k_png_scan's 256 threads
    take two each."""
    base = jpeg_cases.gradient_noise(2, 2731, 3)
    return np.stack([np.roll(base, 7 * i, axis=1) * np.float32(0.5 + 0.003 * i) for i in range(n)])


def reference_strips(frame, fmt):
    """(samples, [the reference's filtered bytes of every strip])."""
    samples = samples_of(frame, fmt)
    raw, bpp = png_ref.raw_rows(samples)
    _, filtered, _ = png_ref.filter_rows(raw, bpp)
    rps = png_ref.strip_rows(raw.shape[1] + 1)
    return samples, [filtered[y:y + rps].tobytes() for y in range(0, raw.shape[0], rps)]


def check_coder_case(name, case):
    """The case's property, from the reference alone (before the library's bytes are looked at); returns the figures."""
    _, strips = reference_strips(case["frame"], case["fmt"])
    models = [png_ref.dynamic_block_model(png_ref.rle_tokens(s)) for s in strips]
    sizes = [png_ref.strip_chunk_sizes(png_ref.rle_tokens(s), len(s)) for s in strips]
    want = case["want"]
    little = f"{name}: the case proves too little"
    d15 = [max(png_ref.huffman_depths(m["freq"]).values()) for m in models]
    d7 = [max(png_ref.huffman_depths(m["cl_freq"]).values()) for m in models]
    fig = {"depth15": d15, "depth7": d7, "repairs15": [m["repairs15"] for m in models], "repairs7": [m["repairs7"] for m in models],
           "dynamic_minus_stored": [a - b for a, b in sizes]}
    assert all(sum(1 for f in m["cl_freq"] if f) >= 2 for m in models)
    if "depth15" in want:
        assert want["depth15"][0] <= d15[0] <= want["depth15"][1] and sizes[0][0] < sizes[0][1], f"{little}: literal / length depth {d15[0]}"
        assert (d15[0] > 15) == (models[0]["repairs15"] > 0)
    if "bytes" in want:
        assert len(strips[0]) == want["bytes"], f"{little}: {len(strips[0])} bytes"
    if "deepest" in want:
        depth = png_ref.huffman_depths(models[0]["freq"])
        over = {s for s, l in depth.items() if l > 15}
        assert set(want["deepest"]) <= over and any(257 <= s <= 285 for s in over), f"{little}: over 15 bits are {sorted(over)}"
    if "depth7" in want:
        assert want["depth7"][0] <= d7[0] <= want["depth7"][1] and sizes[0][0] < sizes[0][1] and models[0]["repairs7"] > 0, f"{little}: code-length depth {d7[0]}"
    if "repair7_excess" in want:
        f7 = models[0]["cl_freq"]
        got = png_ref.code_cost(f7, [png_ref.limited_lengths(f7, 7)[0].get(k, 0) for k in range(19)]) - png_ref.package_merge(f7, 7)
        assert got >= want["repair7_excess"], f"{little}: the repaired 7-bit code is {got} bits over the optimal one"
    if "used" in want:
        used = sum(1 for f in models[0]["freq"] if f)
        assert used == want["used"], f"{little}: {used} used symbols"
    if "dynamic" in want:
        assert (sizes[0][0] < sizes[0][1]) == want["dynamic"], little
    if "decision" in want:
        assert sizes[0][0] - sizes[0][1] == want["decision"], f"{little}: dynamic - stored = {sizes[0][0] - sizes[0][1]} bytes, wanted {want['decision']}"
    if "runs" in want:
        found, at258 = set(), False
        for s in strips:
            assert s[0] == 0 and all(s[k] == 0 for k in range(0, len(s), 8191)), f"{little}: a filter other than None won"
            for end, T in png_ref.runs_of(s):
                found.add((T, end % 64))
                at258 |= T > 258 and (end - T + 258) % 64 == 63
        missing = [(T, lane) for T in RUN_T for lane in RUN_LANES if (T, lane) not in found]
        assert not missing, f"{little}: no run of (T, end lane) {missing}"
        assert at258, f"{little}: no run whose 258th repeat lies on lane 63 while it goes on"
        assert any(end == len(s) - 1 for s in strips for end, _ in png_ref.runs_of(s)), f"{little}: no run ends on a strip's last byte"
        assert any(end > 8191 > end - T for end, T in png_ref.runs_of(strips[0])), f"{little}: no run crosses a row's filter byte"
        assert any(a[-1] == b[0] == b[1] for a, b in zip(strips, strips[1:])), f"{little}: no run crosses a strip boundary"
        assert all(png_ref.rle_tokens(s)[0] == s[0] for s in strips)
        fig["runs"] = sorted(found)
    return fig
