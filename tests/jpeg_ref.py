"""Reference arithmetic and a strict baseline-JPEG parser for the encoder tests (tests/test_emu_jpeg.py, tests/test_gpu_jpeg.py).

Written from ITU-T T.81 and the JFIF convention; imports nothing from sage_gs.

    reference_coefficients(rgb_u8, quality, subsampling)   items 1-6 of the encoder's specification (include/sage_gs.h) in fp64
    parse_jpeg(data)                                       marker segments -> quantised coefficients; raises JpegError on any
                                                           structural fault
    check_coefficients(parsed, ref)                        the comparison rule of the tests
"""
from __future__ import annotations

import numpy as np

# T.81 Annex K.1 / K.2 (natural order) ------------------------------------------------------------------------------------------------
Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                  80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                  95, 98, 112, 100, 103, 99]).reshape(8, 8)
Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                  99, 99] + [99] * 32).reshape(8, 8)
# Figure A.6: natural index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
# Annex K.3 - K.6: (BITS, HUFFVAL) by (class, destination): class 0 = DC, 1 = AC; destination 0 = luminance, 1 = chrominance
_AC_LUM = [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
           36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
           73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
           132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
           178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
           217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250]
_AC_CHR = [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
           21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71,
           72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
           131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
           170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
           216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250]
ANNEX_K_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUM),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHR),
}

W_TIE = 0.002          # unquantised coefficient units: the fp32 error budget of colour conversion + DCT, with a factor of four to spare


class JpegError(ValueError):
    pass


def ijg_table(base, quality):
    """The IJG scaling of an Annex K table: 5000 / q below 50, 200 - 2 q from 50 on; (t * s + 50) / 100 clamped to 1..255."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def _dct_matrix():
    x = np.arange(8)
    c = np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16.0) * 0.5
    c[0] *= np.sqrt(0.5)
    return c                                   # [u][x]


def reference_coefficients(rgb_u8, quality, subsampling):
    """Per component (Y, Cb, Cr): (quotients F / Q float64 [by, bx, 8, 8], rounded int64 of the same shape), natural order [v][u]."""
    rgb = np.asarray(rgb_u8)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    s420 = {"4:2:0": True, "4:4:4": False}[subsampling]
    mcu = 16 if s420 else 8
    H, W = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    p = np.pad(rgb.astype(np.float64), ((0, H - h), (0, W - w), (0, 0)), mode="edge")          # replicate the last column / row
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    planes = [0.299 * r + 0.587 * g + 0.114 * b - 128.0,
              -0.168736 * r - 0.331264 * g + 0.5 * b,
              0.5 * r - 0.418688 * g - 0.081312 * b]
    if s420:
        for i in (1, 2):
            c = planes[i]
            planes[i] = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) / 4.0
    C = _dct_matrix()
    out = []
    for i, pl in enumerate(planes):
        q = ijg_table(Q_LUM if i == 0 else Q_CHR, quality).astype(np.float64)
        blocks = pl.reshape(pl.shape[0] // 8, 8, pl.shape[1] // 8, 8).transpose(0, 2, 1, 3)         # [by, bx, y, x]
        F = np.einsum("vy,abyx,ux->abvu", C, blocks, C)
        quot = F / q
        out.append((quot, (np.sign(quot) * np.floor(np.abs(quot) + 0.5)).astype(np.int64)))
    return out


def tie_window(quot, quality, comp):
    """True where a quotient lies within W_TIE / Q of a rounding tie."""
    q = ijg_table(Q_LUM if comp == 0 else Q_CHR, quality).astype(np.float64)
    frac = np.abs(quot) - np.floor(np.abs(quot))
    return np.abs(frac - 0.5) <= W_TIE / q


def window_share(ref, quality):
    n = sum(r[0].size for r in ref)
    return sum(int(tie_window(r[0], quality, i).sum()) for i, r in enumerate(ref)) / n


def check_coefficients(parsed, ref, quality):
    """Every coefficient of the file equals the reference's, except that one whose fp64 quotient is within W_TIE / Q of a tie may
    differ by one.  Returns (coefficients that differ, coefficients)."""
    n_diff = n = 0
    for i, (quot, want) in enumerate(ref):
        got = parsed["coefficients"][i]
        assert got.shape == want.shape, (i, got.shape, want.shape)
        d = got - want
        win = tie_window(quot, quality, i)
        bad = (d != 0) & ~(win & (np.abs(d) == 1))
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"component {i}: {int(bad.sum())} coefficients differ outside the tie window; first at (by, bx, v, u) = {at}: "
                                 f"file {int(got[at])}, reference {int(want[at])} (quotient {float(quot[at]):.6f})")
        n_diff += int((d != 0).sum()); n += d.size
    return n_diff, n


# ---- the parser ---------------------------------------------------------------------------------------------------------------------
def _huff_lut(bits, vals):
    """16-bit look-ahead table: window -> (symbol, length); length 0 = no code starts with these bits (T.81 Annex C codes)."""
    if len(bits) != 16 or sum(bits) != len(vals):
        raise JpegError("DHT: BITS and HUFFVAL disagree")
    sym = np.zeros(65536, np.int32); ln = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= (1 << length):
                raise JpegError("DHT: more codes than the code space holds")
            lo = code << (16 - length)
            sym[lo:lo + (1 << (16 - length))] = vals[k]; ln[lo:lo + (1 << (16 - length))] = length
            code += 1; k += 1
        code <<= 1
    return sym.tolist(), ln.tolist()


def _segments(data):
    """[(marker, payload offset, payload length)] up to and including SOS; then the offset where entropy-coded data starts."""
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    i, segs = 2, []
    while True:
        if i + 4 > len(data) or data[i] != 0xFF:
            raise JpegError(f"marker expected at {i}")
        m = data[i + 1]
        L = (data[i + 2] << 8) | data[i + 3]
        if L < 2 or i + 2 + L > len(data):
            raise JpegError(f"segment {m:#x} at {i}: bad length {L}")
        segs.append((m, i + 4, L - 2))
        i += 2 + L
        if m == 0xDA:
            return segs, i


def parse_jpeg(data):
    """A baseline (SOF0, Huffman, 8-bit, interleaved single scan) file down to its quantised coefficients.  Returns a dict:
    width, height, components [(id, h, v, tq)], scan [(id, td, ta)], qtables {id: [8, 8] natural order}, huffman {(class, id): (BITS,
    HUFFVAL)}, restart_interval, n_restart_markers, coefficients [per component int64 [by, bx, 8, 8]], eoi (offset of the EOI marker),
    markers (in file order).  Raises JpegError on any structural fault."""
    data = bytes(data)
    segs, pos = _segments(data)
    markers = [m for m, _, _ in segs]
    if markers[0] != 0xE0 or data[segs[0][1]:segs[0][1] + 5] != b"JFIF\0" or segs[0][2] != 14:
        raise JpegError("the first segment is not a JFIF APP0")
    qt, hf, sof, sos, ri = {}, {}, None, None, 0
    for m, o, n in segs:
        seg = data[o:o + n]
        if m == 0xDB:
            if n % 65:
                raise JpegError("DQT: length is not a multiple of 65 (8-bit tables)")
            for k in range(0, n, 65):
                if seg[k] >> 4 or (seg[k] & 15) > 3:
                    raise JpegError("DQT: not an 8-bit table / bad id")
                t = np.zeros(64, np.int64); t[ZIGZAG] = list(seg[k + 1:k + 65])
                qt[seg[k] & 15] = t.reshape(8, 8)
        elif m == 0xC4:
            k = 0
            while k < n:
                if k + 17 > n:
                    raise JpegError("DHT: truncated")
                tc, th = seg[k] >> 4, seg[k] & 15
                bits = list(seg[k + 1:k + 17]); cnt = sum(bits)
                if tc > 1 or th > 1 or k + 17 + cnt > n:
                    raise JpegError("DHT: bad class / id / length")
                hf[(tc, th)] = (bits, list(seg[k + 17:k + 17 + cnt]))
                k += 17 + cnt
        elif m == 0xC0:
            if sof is not None or sos is not None:
                raise JpegError("a second SOF0, or SOF0 after SOS")
            if n < 6 or n != 6 + 3 * seg[5] or seg[0] != 8:
                raise JpegError("SOF0: bad length or precision")
            sof = {"height": (seg[1] << 8) | seg[2], "width": (seg[3] << 8) | seg[4],
                   "components": [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]}
        elif m == 0xDD:
            if n != 2:
                raise JpegError("DRI: bad length")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if sof is None:
                raise JpegError("SOS before SOF0")
            if n < 4 or n != 4 + 2 * seg[0]:
                raise JpegError("SOS: bad length")
            ns = seg[0]
            sos = [(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            if tuple(seg[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise JpegError("SOS: not a baseline scan (Ss, Se, Ah/Al)")
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        else:
            raise JpegError(f"marker {m:#x} has no place in a baseline file")
    if sof["width"] < 1 or sof["height"] < 1:
        raise JpegError("SOF0: empty frame")
    comps = sof["components"]
    if [c[0] for c in comps] != [s[0] for s in sos]:
        raise JpegError("the scan's components are not the frame's")
    for (_, hs, vs, tq), (_, td, ta) in zip(comps, sos):
        if tq not in qt or (0, td) not in hf or (1, ta) not in hf or not (1 <= hs <= 2 and 1 <= vs <= 2):
            raise JpegError("a component names a table that is not defined, or a sampling factor outside 1..2")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus_x, mcus_y = -(-sof["width"] // (8 * hmax)), -(-sof["height"] // (8 * vmax))
    n_mcu = mcus_x * mcus_y
    luts = {k: _huff_lut(*v) for k, v in hf.items()}
    coef = [np.zeros((mcus_y * vs, mcus_x * hs, 64), np.int64) for _, hs, vs, _ in comps]

    # entropy-coded segments: split at markers (0xFF followed by anything but 0x00)
    chunks, start, i, n_rst = [], pos, pos, 0
    while True:
        j = data.find(b"\xff", i)
        if j < 0 or j + 1 >= len(data):
            raise JpegError("no EOI")
        nxt = data[j + 1]
        if nxt == 0x00:
            i = j + 2
            continue
        chunks.append(data[start:j])
        if nxt == 0xD9:
            eoi = j
            break
        if not 0xD0 <= nxt <= 0xD7:
            raise JpegError(f"marker {nxt:#x} inside the scan at {j}")
        if ri == 0:
            raise JpegError("a restart marker without a DRI segment")
        if nxt - 0xD0 != n_rst % 8:
            raise JpegError(f"RST{nxt - 0xD0} at {j}, expected RST{n_rst % 8}")
        n_rst += 1
        start = i = j + 2
    per = ri if ri else n_mcu
    if len(chunks) != -(-n_mcu // per):
        raise JpegError(f"{len(chunks)} entropy-coded segments for {n_mcu} MCUs at a restart interval of {ri}")

    m = 0
    for chunk in chunks:
        raw = chunk.replace(b"\xff\x00", b"\xff")
        bits = np.unpackbits(np.frombuffer(raw + b"\xff\xff", np.uint8)).astype(np.int64)
        nb = 8 * len(raw)
        win = np.zeros(nb + 1, np.int64)
        for k in range(16):
            win += bits[k:k + nb + 1] << (15 - k)
        win = win.tolist()
        p = 0
        pred = [0] * len(comps)
        for _ in range(min(per, n_mcu - m)):
            mx, my = m % mcus_x, m // mcus_x
            for ci, ((_, hs, vs, _), (_, td, ta)) in enumerate(zip(comps, sos)):
                dsym, dlen = luts[(0, td)]
                asym, alen = luts[(1, ta)]
                for by in range(vs):
                    for bx in range(hs):
                        blk = coef[ci][my * vs + by, mx * hs + bx]
                        if p > nb:
                            raise JpegError("the entropy-coded segment ends inside a block")
                        w = win[p]; ln = dlen[w]
                        if ln == 0:
                            raise JpegError(f"a DC code that is not in the table (MCU {m})")
                        size = dsym[w]; p += ln
                        if size > 11:
                            raise JpegError("DC size category above 11")
                        if size:
                            if p > nb:
                                raise JpegError("the entropy-coded segment ends inside a symbol")
                            v = win[p] >> (16 - size); p += size
                            if v < (1 << (size - 1)):
                                v -= (1 << size) - 1
                            pred[ci] += v
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            if p > nb:
                                raise JpegError("the entropy-coded segment ends inside a block")
                            w = win[p]; ln = alen[w]
                            if ln == 0:
                                raise JpegError(f"an AC code that is not in the table (MCU {m})")
                            rs = asym[w]; p += ln
                            run, size = rs >> 4, rs & 15
                            if size == 0:
                                if run == 15:
                                    k += 16
                                    if k > 64:
                                        raise JpegError("ZRL runs past the block")
                                    continue
                                if run != 0:
                                    raise JpegError("EOBn in a baseline scan")
                                break
                            k += run
                            if k > 63 or size > 10:
                                raise JpegError("an AC run past the block / size above 10")
                            if p > nb:
                                raise JpegError("the entropy-coded segment ends inside a symbol")
                            v = win[p] >> (16 - size); p += size
                            if v < (1 << (size - 1)):
                                v -= (1 << size) - 1
                            blk[ZIGZAG[k]] = v
                            k += 1
            m += 1
        if p > nb:
            raise JpegError("the entropy-coded segment ends inside a symbol")
        if nb - p >= 8:
            raise JpegError(f"{(nb - p) // 8} bytes left over at the end of an entropy-coded segment")
        if nb - p and not bits[p:nb].all():
            raise JpegError("padding bits that are not ones")
    return {"width": sof["width"], "height": sof["height"], "components": comps, "scan": sos, "qtables": qt, "huffman": hf,
            "restart_interval": ri, "n_restart_markers": n_rst, "eoi": eoi, "markers": markers,
            "coefficients": [c.reshape(c.shape[0], c.shape[1], 8, 8) for c in coef]}
