"""The PNG encoder's reference, in NumPy / zlib / struct: the samples and the filter choice of include/sage_gs.h restated, a chunk
parser, and the strip geometry.  Nothing here looks at the library."""
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
