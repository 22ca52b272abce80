"""The PNG encoder's reference, in NumPy / zlib / struct: the samples and the filter choice of include/sage_gs.h restated, a chunk
parser, the strip geometry, and the deflate coder's reference (the run parse, optimal and length-limited code costs, a bit-level
reader of a strip's stream, the documented construction of a dynamic block restated).  Nothing here looks at the library."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
STRIP = 16384                      # filtered bytes per strip
FILTER_NAMES = ("None", "Sub", "Up", "Average", "Paeth")


class PngError(ValueError):
    pass


def rgb_samples(rgb_f32):
    """uint8 [H,W,3]: clamp to [0,1], (unsigned)(x * 255 + 0.5), every step in fp32 (k_pack_rgba8's level, each step rounded)."""
    x = np.clip(np.asarray(rgb_f32, np.float32), np.float32(0), np.float32(1))
    return (x * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def depth_samples(depth_f32, depth_scale=10000.0, depth_max=6.5):
    """uint16 [H,W]: np.clip(d, 0, max) * scale -> astype(uint16) in fp32 (vlm_client_modular.py:355-356), NaN defined as 0."""
    d = np.asarray(depth_f32, np.float32)
    d = np.where(np.isnan(d), np.float32(0), d)
    c = np.clip(d, np.float32(0), np.float32(depth_max))
    return (c * np.float32(depth_scale)).astype(np.uint16)


def raw_rows(samples):
    """uint8 [H, row bytes] of uint8 [H,W,3] or uint16 [H,W] samples (16-bit samples big-endian); bytes per pixel."""
    s = np.asarray(samples)
    if s.dtype == np.uint8 and s.ndim == 3 and s.shape[2] == 3:
        return np.ascontiguousarray(s).reshape(s.shape[0], -1), 3
    if s.dtype == np.uint16 and s.ndim == 2:
        return np.ascontiguousarray(s.astype(">u2")).view(np.uint8).reshape(s.shape[0], -1), 2
    raise ValueError("samples must be uint8 [H,W,3] or uint16 [H,W]")


def filter_candidates(row, prev, bpp):
    """The five filtered versions of a raw row (int arrays mod 256) given the raw row above it."""
    cur = row.astype(np.int32); up = prev.astype(np.int32)
    a = np.zeros_like(cur); c = np.zeros_like(cur)        # the pixel to the left, and the one above it: zeros left of the first pixel
    a[bpp:] = cur[:-bpp]; c[bpp:] = up[:-bpp]
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    return [(cur - pred) & 255 for pred in (np.zeros_like(cur), a, up, (a + up) >> 1, paeth)]


def filter_rows(raw, bpp):
    """(filter type per row, filtered uint8 [H, 1 + row bytes]): per row the filter with the least sum of |byte read as signed|, ties to
    the lowest type; the row above the first is zeros."""
    h, nb = raw.shape
    out = np.zeros((h, nb + 1), np.uint8)
    types, tied = [], []
    prev = np.zeros(nb, np.uint8)
    for y in range(h):
        cands = filter_candidates(raw[y], prev, bpp)
        sums = [int(np.where(f < 128, f, 256 - f).sum()) for f in cands]
        ft = int(np.argmin(sums))                           # the first of equal minima
        tied.append(sums.count(sums[ft]) > 1)
        types.append(ft)
        out[y, 0] = ft; out[y, 1:] = cands[ft]
        prev = raw[y]
    return types, out, tied


def strip_rows(row_len):
    """Rows per strip of filtered rows of row_len bytes (1 + row bytes)."""
    return max(1, STRIP // row_len)


def parse_png(data):
    """{'chunks': [(type, payload)], 'ihdr': (w, h, bit depth, colour type, compression, filter, interlace)}; raises PngError on a bad
    signature, a chunk running past the end, a wrong CRC, or bytes after IEND."""
    if data[:8] != SIGNATURE:
        raise PngError("signature")
    at, chunks = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise PngError(f"truncated chunk at {at}")
        n, = struct.unpack(">I", data[at:at + 4])
        typ = data[at + 4:at + 8]
        if at + 12 + n > len(data):
            raise PngError(f"chunk {typ!r} at {at} runs past the end")
        body = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if crc != zlib.crc32(typ + body):
            raise PngError(f"CRC of chunk {typ!r} at {at}: file {crc:08x}, zlib.crc32 {zlib.crc32(typ + body):08x}")
        chunks.append((typ, body))
        at += 12 + n
        if typ == b"IEND":
            break
    if at != len(data):
        raise PngError(f"{len(data) - at} bytes after IEND")
    if not chunks or chunks[0][0] != b"IHDR" or len(chunks[0][1]) != 13:
        raise PngError("IHDR")
    return {"chunks": chunks, "ihdr": struct.unpack(">IIBBBBB", chunks[0][1])}


def zlib_rle_strip(filtered_bytes):
    """Bytes of one strip deflated alone by zlib at level 1 with run matches only, ended by a sync flush (the empty stored block)."""
    z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    return len(z.compress(filtered_bytes) + z.flush(zlib.Z_SYNC_FLUSH))


def zlib_rle_file_size(filtered, n_strips, rows_per_strip):
    """The file zlib would make of the same filtered bytes on the same strips with the same framing: signature + IHDR + IEND + zlib
    header + final block + Adler-32 = 56 bytes, 12 per chunk."""
    total = 56
    for s in range(n_strips):
        total += 12 + zlib_rle_strip(filtered[s * rows_per_strip:(s + 1) * rows_per_strip].tobytes())
    return total


# ---- the deflate coder's reference: the run parse, optimal and length-limited code costs, a bit-level reader ---------------------------
# A token is a literal 0..255 or 256 + the length of a match at distance 1.
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def rle_tokens(strip_bytes):
    """The tokens of one strip as csrc/sgs_png.h's header comment and zlib's Z_RLE state them: a run's first byte is a literal, the
    repeats after it go greedily into matches of distance 1 and length up to 258, a remainder of 1 or 2 repeats is literals; nothing
    matches back across the strip's first byte."""
    b = bytes(strip_bytes)
    out, i, n = [], 0, len(b)
    while i < n:
        v = b[i]
        j = i + 1
        while j < n and b[j] == v:
            j += 1
        out.append(v)
        rep = j - i - 1
        while rep >= 258:
            out.append(256 + 258); rep -= 258
        if rep >= 3:
            out.append(256 + rep)
        else:
            out.extend([v] * rep)
        i = j
    return out


def runs_of(strip_bytes):
    """[(index of the run's last byte, its number of repeats T)] for every byte that equals the one before it and not the one after."""
    b = bytes(strip_bytes)
    out, start = [], 0
    for i in range(1, len(b) + 1):
        if i == len(b) or b[i] != b[i - 1]:
            if i - 1 > start:
                out.append((i - 1, i - 1 - start))
            start = i
    return out


def length_symbol(length):
    """(symbol 257..285, number of extra bits) of a match length 3..258."""
    for k in range(28, -1, -1):
        if length >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k]
    raise ValueError(length)


def token_histogram(tokens):
    """Frequencies of the 286 literal / length symbols of a token list, the end-of-block symbol included; the extra and distance bits
    the matches take (one distance bit each: the one-bit code of distance 1)."""
    freq, other = [0] * 286, 0
    for t in tokens:
        if t < 256:
            freq[t] += 1
        else:
            s, e = length_symbol(t - 256)
            freq[s] += 1
            other += e + 1
    freq[256] += 1
    return freq, other


def huffman_depths(freqs):
    """Code lengths of the unconstrained optimal code of the non-zero frequencies (a heap; equal weights: leaves before inner nodes,
    older before newer — the optimal code of the least depth).  {index: length}; one used symbol gets length 1."""
    import heapq
    used = [(f, 0, i, (i,)) for i, f in enumerate(freqs) if f]
    if len(used) == 1:
        return {used[0][2]: 1}
    depth = {u[2]: 0 for u in used}
    heap = list(used)
    heapq.heapify(heap)
    seq = len(freqs)
    while len(heap) > 1:
        a = heapq.heappop(heap); b = heapq.heappop(heap)
        for i in a[3] + b[3]:
            depth[i] += 1
        seq += 1
        heapq.heappush(heap, (a[0] + b[0], 1, seq, a[3] + b[3]))
    return depth


def code_cost(freqs, lengths):
    return sum(f * lengths[i] for i, f in enumerate(freqs) if f)


def package_merge(freqs, limit):
    """Bits of the optimal code of the non-zero frequencies with no length over `limit` (Larmore & Hirschberg's package-merge: the
    cost is the weight of the 2n - 2 cheapest items of the last merge)."""
    fs = sorted(f for f in freqs if f)
    n = len(fs)
    if n == 1:
        return fs[0]
    if n > (1 << limit):
        raise ValueError(f"{n} symbols do not fit {limit} bits")
    cur = list(fs)
    for _ in range(limit - 1):
        cur = sorted(fs + [cur[2 * i] + cur[2 * i + 1] for i in range(len(cur) // 2)])
    return sum(cur[:2 * n - 2])


def package_merge_lengths(freqs, limit):
    """{index: length} of an optimal code with no length over `limit`: package-merge with the items' contents kept (each item is
    the list of the leaves in it, a leaf once per level it was taken at)."""
    order = sorted((i for i, f in enumerate(freqs) if f), key=lambda i: (freqs[i], i))
    n = len(order)
    if n == 1:
        return {order[0]: 1}
    leaves = [(freqs[i], 0, k, (i,)) for k, i in enumerate(order)]
    cur = list(leaves)
    for _ in range(limit - 1):
        packs = [(cur[2 * k][0] + cur[2 * k + 1][0], 1, k, cur[2 * k][3] + cur[2 * k + 1][3]) for k in range(len(cur) // 2)]
        cur = sorted(leaves + packs)[:2 * n - 2]
    out = {i: 0 for i in order}
    for item in cur[:2 * n - 2]:
        for i in item[3]:
            out[i] += 1
    return out


def kraft(lengths, limit):
    """Sum of 2^(limit - length) over the non-zero lengths: 2^limit for a complete code."""
    return sum(1 << (limit - l) for l in lengths if l)


class _Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def get(self, n):
        if self.pos + n > 8 * len(self.d):
            raise PngError(f"the stream ends inside a field at bit {self.pos}")
        v = 0
        for k in range(n):
            p = self.pos + k
            v |= ((self.d[p >> 3] >> (p & 7)) & 1) << k
        self.pos += n
        return v


def _decoder(lengths, limit, what, may_be_partial=False):
    """{(length, code): symbol} of a canonical code; PngError on a length over the limit, an over-subscribed or an incomplete code
    (may_be_partial: no code at all, or a single code of one bit, is accepted — RFC 1951's distance code of one distance)."""
    if any(l > limit for l in lengths):
        raise PngError(f"{what}: a length of {max(lengths)} bits (limit {limit})")
    used = [l for l in lengths if l]
    k = kraft(lengths, limit)
    if k > (1 << limit):
        raise PngError(f"{what}: over-subscribed code (Kraft sum {k} / {1 << limit})")
    if k < (1 << limit) and not (may_be_partial and (not used or used == [1])):
        raise PngError(f"{what}: incomplete code (Kraft sum {k} / {1 << limit})")
    count = [0] * (limit + 2)
    for l in used:
        count[l] += 1
    nxt, code = [0] * (limit + 2), 0
    for l in range(1, limit + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table, limit, what):
    code = 0
    for l in range(1, limit + 1):
        code = (code << 1) | bits.get(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise PngError(f"{what}: a code that is not in the table at bit {bits.pos}")


def parse_deflate(raw_stream):
    """The blocks of a raw deflate stream (a strip's: it ends byte-aligned, with or without a final block), read bit by bit.  Per block
    a dict: type (0 stored, 1 fixed, 2 dynamic), final, bits (the block's size), tokens; a dynamic block also hlit, hdist, hclen,
    cl_lengths (19, by symbol), cl_symbols (the run-length coded length sequence as it stands in the header), litlen_lengths,
    dist_lengths, header_bits; a stored block data.  Raises PngError on an over-subscribed or incomplete code, a length over 15 (7 for
    the code of the code lengths), a repeat code with nothing before it or running past the lengths, a missing end-of-block code, a
    code not in the table, a distance other than 1 or reaching before the strip's first byte, a stored block with LEN != ~NLEN, a
    reserved block type, a stream that ends inside a block and bytes after the final block."""
    bits = _Bits(raw_stream)
    blocks, produced = [], 0
    while True:
        if bits.pos == 8 * len(bits.d):
            break
        start = bits.pos
        final, typ = bits.get(1), bits.get(2)
        blk = {"type": typ, "final": final, "tokens": []}
        if typ == 3:
            raise PngError("reserved block type 3")
        if typ == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.get(16), bits.get(16)
            if n != (~nn & 0xFFFF):
                raise PngError(f"stored block: LEN {n:#06x} is not the complement of NLEN {nn:#06x}")
            at = bits.pos >> 3
            if at + n > len(bits.d):
                raise PngError("stored block runs past the end of the stream")
            blk["data"] = bits.d[at:at + n]
            blk["tokens"] = list(blk["data"])
            bits.pos += 8 * n
            produced += n
        else:
            if typ == 1:
                lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dist = [5] * 32                             # symbols 30 and 31 take part in the code and never occur
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                if hlit > 286 or hdist > 30:
                    raise PngError(f"HLIT {hlit} / HDIST {hdist}")
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.get(3)
                cl_table = _decoder(cl, 7, "code of the code lengths")
                seq, syms = [], []
                while len(seq) < hlit + hdist:
                    s = _symbol(bits, cl_table, 7, "code of the code lengths")
                    syms.append(s)
                    if s < 16:
                        seq.append(s)
                        continue
                    if s == 16:
                        if not seq:
                            raise PngError("repeat code 16 with nothing before it")
                        v, rep = seq[-1], 3 + bits.get(2)
                    else:
                        v, rep = 0, (3 + bits.get(3)) if s == 17 else (11 + bits.get(7))
                    if len(seq) + rep > hlit + hdist:
                        raise PngError("a repeat code runs past the last code length")
                    seq.extend([v] * rep)
                lit, dist = seq[:hlit], seq[hlit:]
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=cl, cl_symbols=syms, litlen_lengths=lit, dist_lengths=dist,
                           header_bits=bits.pos - start)
                if not lit[256]:
                    raise PngError("no end-of-block code")
            lit_table = _decoder(lit, 15, "literal / length code")
            dist_table = _decoder(dist, 15, "distance code", may_be_partial=True)
            while True:
                s = _symbol(bits, lit_table, 15, "literal / length code")
                if s < 256:
                    blk["tokens"].append(s); produced += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise PngError(f"length symbol {s}")
                    length = LEN_BASE[s - 257] + bits.get(LEN_EXTRA[s - 257])
                    ds = _symbol(bits, dist_table, 15, "distance code")
                    if ds > 29:
                        raise PngError(f"distance symbol {ds}")
                    d = DIST_BASE[ds] + bits.get(DIST_EXTRA[ds])
                    if d > produced:
                        raise PngError(f"a match at distance {d} after {produced} bytes reaches before the strip")
                    if d != 1:
                        raise PngError(f"a match at distance {d}: only runs (distance 1) are coded")
                    blk["tokens"].append(256 + length); produced += length
        blk["bits"] = bits.pos - start
        blocks.append(blk)
        if final:
            if ((bits.pos + 7) >> 3) != len(bits.d):
                raise PngError("bytes after the final block")
            break
    return blocks


def expand_tokens(tokens):
    """The bytes a token list stands for."""
    out = bytearray()
    for t in tokens:
        if t < 256:
            out.append(t)
        else:
            if not out:
                raise PngError("a match before any byte")
            out.extend(out[-1:] * (t - 256))
    return bytes(out)


def zlib_rle_stream(strip_bytes):
    """zlib's own raw stream of one strip: level 1, run matches only, ended by a sync flush."""
    z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    return z.compress(bytes(strip_bytes)) + z.flush(zlib.Z_SYNC_FLUSH)


# ---- the documented construction of a strip's dynamic block, restated: what the block takes ---------------------------------------------
def limited_lengths(freqs, limit):
    """{index: length}: the optimal lengths (huffman_depths), lengths over the limit folded to it and the Kraft sum repaired by
    lengthening one code of the deepest shorter length per step; the longest lengths go to the rarest symbols, ties by index."""
    depth = huffman_depths(freqs)
    num = [0] * (limit + 1)
    for l in depth.values():
        num[min(l, limit)] += 1
    total = sum(num[l] << (limit - l) for l in range(1, limit + 1))
    steps = 0
    while total > (1 << limit):
        num[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if num[l]:
                num[l] -= 1; num[l + 1] += 2
                break
        total -= 1
        steps += 1
    order = sorted(depth, key=lambda i: (freqs[i], i))
    out, j = {}, 0
    for l in range(limit, 0, -1):
        for _ in range(num[l]):
            out[order[j]] = l; j += 1
    return out, steps


def length_sequence_symbols(seq):
    """The code-length symbols of a sequence of code lengths: (symbol, extra bits' count) — zeros in runs of 11..138 (18) and 3..10
    (17), a non-zero length once and its repeats in groups of 3..6 (16), what is left over plainly."""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138); out.append((18, 7)); run -= r
            if run >= 3:
                out.append((17, 3)); run = 0
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, 2)); run -= r
        out.extend([(v, 0)] * run)
    return out


def dynamic_block_model(tokens):
    """What the documented construction makes of a token list: dict(litlen, cl (lengths), hlit, hclen, header_bits, body_bits,
    repairs15, repairs7, cl_freq)."""
    freq, other = token_histogram(tokens)
    lit, rep15 = limited_lengths(freq, 15)
    hlit = max(257, max(lit) + 1)
    seq = [lit.get(s, 0) for s in range(hlit)] + [1]
    syms = length_sequence_symbols(seq)
    cl_freq = [0] * 19
    for s, _ in syms:
        cl_freq[s] += 1
    true_cl_freq = list(cl_freq)
    if sum(1 for f in cl_freq if f) < 2:
        cl_freq[1 if cl_freq[0] else 0] = 1
    cl, rep7 = limited_lengths(cl_freq, 7)
    if rep7:                                               # the code of the code lengths is not repaired: the optimal 7-bit code takes its place
        cl = package_merge_lengths(cl_freq, 7)
    hclen = 19
    while hclen > 4 and CL_ORDER[hclen - 1] not in cl:
        hclen -= 1
    header = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl[s] + e for s, e in syms)
    body = sum(f * lit[s] for s, f in enumerate(freq) if f) + other
    return {"litlen": lit, "cl": cl, "hlit": hlit, "hclen": hclen, "header_bits": header, "body_bits": body, "repairs15": rep15,
            "repairs7": rep7, "cl_freq": true_cl_freq, "freq": freq}


def strip_chunk_sizes(tokens, n_bytes):
    """(bytes the dynamic coding of the strip takes, bytes the stored one takes): the block, then the empty stored block that aligns."""
    m = dynamic_block_model(tokens)
    return ((m["header_bits"] + m["body_bits"] + 3 + 7) >> 3) + 4, 5 + n_bytes + 5
