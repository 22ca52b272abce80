"""The PNG encoder's checks, shared by the CPU-emulator tests (test_emu_png.py) and the GPU tests (test_gpu_png.py): the picture set, a
driver of the C ABI over plain buffers, and the assertions on a file (lossless, structure, filters, sizes, against zlib on the same
strips)."""
from __future__ import annotations

import ctypes as C
import io
import zlib

import numpy as np

import jpeg_cases
import png_ref

SENTINEL = 0xA5
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


class AbiPng:
    """sgs_encode_png over host buffers (the emulator's 'device' is the host).  A GPU driver overrides the four buffer hooks."""

    def __init__(self, lib, ctx=None):
        from sage_gs import _capi
        self._capi, self.lib = _capi, lib
        self.ctx, self._own = ctx, ctx is None
        if ctx is None:
            self.ctx = C.c_void_p()
            lib.check(lib.sgs_create(0, _capi.BACKEND_HIP, C.byref(self.ctx)))

    def close(self):
        if self._own and self.ctx:
            self.lib.sgs_destroy(self.ctx)
            self.ctx = None

    # buffer hooks: (object that keeps the memory alive, address[, getter of a host copy])
    def _frames(self, frames):
        a = np.ascontiguousarray(frames, np.float32)
        return a, a.ctypes.data

    def _bytes(self, n):
        a = np.full(n, SENTINEL, np.uint8)
        return a, a.ctypes.data, lambda: a

    def _i64(self, n):
        a = np.full(n, -1, np.int64)
        return a, a.ctypes.data, lambda: a

    def _sync(self):
        pass

    def bound(self, w, h, fmt="rgb8", depth_scale=10000.0, depth_max=6.5):
        p = self._capi.png_params(fmt, depth_scale, depth_max)
        return int(self.lib.sgs_png_bound(int(w), int(h), C.byref(p)))

    def encode(self, frames, fmt="rgb8", capacity=None, slack=64, depth_scale=10000.0, depth_max=6.5):
        """frames fp32 [n,H,W,3] (rgb8) or [n,H,W] (depth16).  Returns dict(files, offsets, sizes, buffer (capacity + slack bytes,
        SENTINEL-filled before the call), capacity, rc (sgs_png_status after synchronising), needed)."""
        frames = np.asarray(frames, np.float32)
        n, h, w = frames.shape[:3]
        p = self._capi.png_params(fmt, depth_scale, depth_max)
        cap = n * self.bound(w, h, fmt, depth_scale, depth_max) if capacity is None else int(capacity)
        keep_f, f_ptr = self._frames(frames)
        keep_o, o_ptr, o_get = self._bytes(cap + slack)
        keep_a, a_ptr, a_get = self._i64(n)
        keep_s, s_ptr, s_get = self._i64(n)
        self.lib.check(self.lib.sgs_encode_png(self.ctx, f_ptr, w, h, n, int(np.prod(frames.shape[1:])), C.byref(p), o_ptr, cap, a_ptr, s_ptr, None),
                       self.ctx)
        self._sync()
        need = C.c_int64(-1)
        rc = int(self.lib.sgs_png_status(self.ctx, C.byref(need)))
        buf, offs, sizes = o_get(), a_get(), s_get()
        files = [bytes(buf[int(o):int(o) + int(z)]) for o, z in zip(offs, sizes)] if rc == 0 else None
        return {"files": files, "offsets": offs, "sizes": sizes, "buffer": buf, "capacity": cap, "rc": rc, "needed": int(need.value)}

    def encode_one(self, frame, fmt="rgb8", **kw):
        r = self.encode(np.asarray(frame, np.float32)[None], fmt, **kw)
        assert r["rc"] == 0, r["rc"]
        jpeg_cases.check_nothing_written_beyond(r)
        return r["files"][0]


def pil_size(samples, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(samples).save(b, "PNG", **kw)
    return len(b.getvalue())


def check_file(data, samples, bound, label="", against_zlib=True):
    """Checks 1-5 on one file against the samples it must hold (uint8 [H,W,3] or uint16 [H,W]); prints and returns the figures.
    against_zlib=False prints check 5's ratio without asserting it (for rows of ten samples beside the picture set, which test sample
    values: a strip of 21 bytes is stored behind 10 bytes of block framing, and zlib's fixed-code block has none)."""
    from PIL import Image
    samples = np.ascontiguousarray(samples)
    raw, bpp = png_ref.raw_rows(samples)
    h, nb = raw.shape
    w = nb // bpp
    # 1 lossless
    im = Image.open(io.BytesIO(data)); im.load()
    assert im.mode == ("RGB" if bpp == 3 else "I;16") and im.size == (w, h), (im.mode, im.size)
    assert np.array_equal(np.asarray(im), samples), f"{label}: PIL reads other samples"
    # 2 structure
    parsed = png_ref.parse_png(data)                        # signature, every CRC, nothing after IEND
    rps = png_ref.strip_rows(nb + 1)
    n_strips = -(-h // rps)
    names = [t for t, _ in parsed["chunks"]]
    assert names == [b"IHDR"] + [b"IDAT"] * n_strips + [b"IEND"], (label, names[:4], len(names), n_strips)
    assert parsed["ihdr"] == (w, h, 8 if bpp == 3 else 16, 2 if bpp == 3 else 0, 0, 0, 0), parsed["ihdr"]
    assert parsed["chunks"][-1][1] == b""
    idat = [b for t, b in parsed["chunks"] if t == b"IDAT"]
    z = zlib.decompressobj()
    inflated = z.decompress(b"".join(idat)) + z.flush()
    assert z.eof and z.unused_data == b"" and len(inflated) == h * (nb + 1), (label, z.eof, len(z.unused_data), len(inflated))
    assert idat[0][:2] == b"\x78\x01"
    # 3 filters (and, with them, every filtered byte)
    types, filtered, tied = png_ref.filter_rows(raw, bpp)
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
            "pil_level1": pil1, "pil_default": pild, "strips": n_strips, "tied_rows": int(sum(tied))}


def check_smaller_than_raw(fig, label, noise=False):
    """Check 4's last item: every picture but noise is smaller than its raw bytes (from SMALLER_THAN_RAW_FROM raw bytes on)."""
    if not noise and fig["raw"] >= SMALLER_THAN_RAW_FROM:
        assert fig["bytes"] < fig["raw"], f"{label}: {fig['bytes']} bytes, raw {fig['raw']}"


def emu_library():
    """The emulator library of csrc/, rebuilt when sgs_png.h is newer than it (emu_harness's own staleness check does not know that
    header)."""
    import os
    import emu_harness
    hdr = os.path.join(emu_harness.PKG, "csrc", "sgs_png.h")
    lib = emu_harness.EMU_LIB
    return emu_harness.build_emu(force=os.path.exists(lib) and os.path.getmtime(hdr) > os.path.getmtime(lib))
