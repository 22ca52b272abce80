"""The frame resize's checks, shared by the CPU-emulator tests (test_emu_resize.py) and the GPU tests (test_gpu_resize.py): the shape
pairs, pictures built for the branches (each with its property, asserted from the restatement alone), a driver of the C ABI over plain
buffers, and the assertions against tests/resize_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

import jpeg_cases
import png_cases
import png_ref
import resize_ref as ref
from abi_driver import AbiDriver, GpuBuffers

# W, H -> w, h
SHAPES = [
    (37, 23, 13, 7),       # odd ratios; windows cut at both edges
    (13, 7, 37, 23),       # enlarging: the support is not scaled
    (64, 48, 32, 24),      # the reference's 2:1
    (96, 54, 16, 12),      # ratios 6 and 4.5 (1080p -> 320x240 in small); 25 taps
    (64, 48, 64, 20),      # the horizontal pass skipped
    (33, 17, 5, 17),       # the vertical pass skipped
    (16, 16, 16, 16),      # both skipped: the quantised frame itself
    (1, 1, 3, 2),          # degenerate sizes
    (5, 4, 1, 1),
]
OVERSHOOT_SHAPES = SHAPES[:4]      # where the checkerboard picture must drive the sum out of [0, 255]
SENTINEL = np.float32(-7.0e8)      # what dst holds before a call, padding included


def shape_id(s):
    return f"{s[0]}x{s[1]}_to_{s[2]}x{s[3]}"


# ---- pictures ---------------------------------------------------------------------------------------------------------------------------
def thresholds(W, H, seed=3):
    """fp32 inputs on, one ulp below and one ulp above the threshold (k - 1/2) / 255 of level k, and inputs below 0 and above 1."""
    rs = np.random.RandomState(seed)
    k = rs.randint(1, 256, (H, W, 3))
    t = ((k - 0.5) / 255.0).astype(np.float32)
    which = rs.randint(0, 5, (H, W, 3))
    out = np.where(which == 0, np.nextafter(t, np.float32(-1)), np.where(which == 1, np.nextafter(t, np.float32(2)), t)).astype(np.float32)
    out = np.where(which == 3, np.float32(-0.3), np.where(which == 4, np.float32(1.7), out)).astype(np.float32)
    return out


def colour_pictures(W, H, cell=3):
    """name -> fp32 [H,W,3], in the order the checks run.  cell: the side of the checkerboard's squares."""
    rs = np.random.RandomState(W * 1000 + H)
    rand = ref.unlevel(rs.randint(0, 256, (H, W, 3)))
    checker = rand.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    top = (((xx // cell) + (yy // cell)) % 2).astype(np.float32)
    checker[:max(H // 2, 1)] = top[:max(H // 2, 1), :, None]
    return {
        "constant_255": np.ones((H, W, 3), np.float32),
        "constant_1": np.full((H, W, 3), ref.unlevel(1), np.float32),
        "thresholds": thresholds(W, H),
        "checker": checker,
        "random": rand,
    }


def depth_pictures(W, H):
    """name -> (fp32 [H,W], clip or None)."""
    rs = np.random.RandomState(W * 77 + H)
    d = (rs.rand(H, W) * 7).astype(np.float32)
    d[::5, ::3] = np.float32(6.5)
    holes = d.copy()
    holes[rs.rand(H, W) < 0.15] = np.inf
    holes[H // 2, W // 2] = np.inf
    nan = d.copy()
    nan[H // 2, W // 3] = np.nan
    return {"plateaus": (d, None), "inf_holes": (holes, (0.1, 6.5)), "single_nan": (nan, None)}


def pictures_of(shape):
    """The colour pictures of a shape pair: the checkerboard's squares are twice the larger ratio wide (at least 3 pixels), so that an
    edge between them is as wide as the filter's support and the cubic's negative lobes show."""
    W, H, w, h = shape
    return colour_pictures(W, H, max(3, 2 * int(np.ceil(max(W / w, H / h)))))


def check_picture_properties(shape):
    """What the pictures are built for, from the restatement alone (before the library is asked)."""
    W, H, w, h = shape
    pics = pictures_of(shape)
    if shape in OVERSHOOT_SHAPES:
        _, (lo, hi) = ref.bicubic_u8(ref.levels(pics["checker"]), w, h, with_range=True)
        assert lo < 0 and hi > 255, f"{shape_id(shape)}: the checkerboard's sums stay within [{lo}, {hi}]: the clamp is not exercised"
    t = pics["thresholds"]
    lv = ref.levels(t)
    up = ref.levels(np.nextafter(t, np.float32(2))).astype(int) - lv
    assert W * H < 16 or ((up == 1).any() and (up == 0).any()), "no input lies one ulp under a level threshold"
    assert W * H < 16 or ((t < 0).any() and (t > 1).any() and lv.min() == 0 and lv.max() == 255)
    assert ref.levels(pics["constant_255"]).min() == 255 and (ref.levels(pics["constant_1"]) == 1).all()
    holes, clip = depth_pictures(W, H)["inf_holes"]
    assert np.isinf(holes).any() and np.isfinite(ref.bicubic_f32(holes, w, h, clip)).all() and np.isfinite(ref.linear_f(holes, w, h, clip)).all()
    nan = depth_pictures(W, H)["single_nan"][0]
    hit = np.isnan(ref.bicubic_f32(nan, w, h))
    assert np.isnan(nan).sum() == 1 and hit.any() and (W * H <= 20 or w * h <= 6 or not hit.all()), "the NaN reaches no pixel, or all of them"


# ---- the C ABI over plain buffers ---------------------------------------------------------------------------------------------------------
class AbiResize(AbiDriver):
    """sgs_resize (and sgs_pack_rgba8) over host buffers; a GPU driver overrides the buffer hooks (GpuResize)."""

    def _floats(self, a):
        a = np.ascontiguousarray(a, np.float32)
        return a, a.ctypes.data, lambda: a

    def call(self, src_ptr, W, H, n, src_stride, params, dst_ptr, dst_stride):
        return int(self.lib.sgs_resize(self.ctx, src_ptr, int(W), int(H), int(n), int(src_stride), C.byref(params) if params is not None else None,
                                       dst_ptr, int(dst_stride), None))

    def resize(self, frames, size, fmt="rgb8", filter="bicubic", clip=None, src_stride=None, dst_stride=None, slack=64):
        """frames fp32 [n,H,W,3] (rgb8) or [n,H,W] (f32) -> dict(out [n,h,w(,3)], buffer: all of dst — SENTINEL before the call —
        with `slack` floats behind the last frame).  Strides in floats (default: a frame); the floats between source frames are NaN
        and 1e30 in turn."""
        frames = np.asarray(frames, np.float32)
        n, H, W = frames.shape[:3]
        w, h = size
        ch = 3 if fmt == "rgb8" else 1
        assert frames.shape[3:] == ((3,) if ch == 3 else ())
        src_floats, dst_floats = H * W * ch, h * w * ch
        ss = src_floats if src_stride is None else int(src_stride)
        ds = dst_floats if dst_stride is None else int(dst_stride)
        lo, hi = (float("-inf"), float("inf")) if clip is None else clip
        p = self._capi.resize_params(fmt, filter, w, h, lo, hi)
        keep_s, s_ptr = self._frames(jpeg_cases.strided(frames, ss))
        keep_d, d_ptr, d_get = self._floats(np.full(max(n - 1, 0) * ds + dst_floats + slack, SENTINEL, np.float32))
        rc = self.call(s_ptr, W, H, n, ss, p, d_ptr, ds)
        self.lib.check(rc, self.ctx)
        self._sync()
        buf = np.array(d_get())
        out = np.stack([buf[i * ds:i * ds + dst_floats].reshape((h, w, 3) if ch == 3 else (h, w)) for i in range(n)])
        return {"out": out, "buffer": buf, "dst_stride": ds, "dst_floats": dst_floats, "n": n}

    def one(self, frame, size, fmt="rgb8", filter="bicubic", clip=None):
        r = self.resize(np.asarray(frame, np.float32)[None], size, fmt, filter, clip)
        check_padding_untouched(r)
        return r["out"][0]

    def pack(self, frame):
        """sgs_pack_rgba8 of an fp32 [h,w,3] frame: uint8 [h,w,3]."""
        h, w = frame.shape[:2]
        keep_f, f_ptr = self._frames(frame)
        keep_o, o_ptr, o_get = self._bytes(h * w * 4)
        self.lib.check(self.lib.sgs_pack_rgba8(self.ctx, f_ptr, o_ptr, w, h, None), self.ctx)
        self._sync()
        rgba = np.array(o_get()).reshape(h, w, 4)
        assert (rgba[..., 3] == 255).all()
        return rgba[..., :3]


class GpuResize(GpuBuffers, AbiResize):
    """AbiResize over torch device buffers, on a Renderer's context."""

    def _floats(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.r.device)
        return t, t.data_ptr(), lambda: t.cpu().numpy()


def check_padding_untouched(r):
    buf, ds, df = r["buffer"], r["dst_stride"], r["dst_floats"]
    for i in range(r["n"]):
        end = (i + 1) * ds if i + 1 < r["n"] else len(buf)
        pad = buf[i * ds + df:end]
        assert (pad == SENTINEL).all(), f"dst was written outside frame {i}: first at float {i * ds + df + int(np.argmax(pad != SENTINEL))}"
    assert not (buf[:df] == SENTINEL).all(), "dst was not written at all"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# The fp32 bilinear value against the same lerps evaluated in fp64, with u = 2^-24 and M the largest sample magnitude after the clip:
# tx = fx / 2w and ty = fy / 2h carry one rounding each — taken as within 1 ulp, 2u relative, should a build's division not round
# correctly.  top = a + (b - a) tx: the difference is at most 2M and its rounding at most 2M u; the product (at most 2M) inherits that,
# 2M 2u from tx and 2M u of its own rounding; the sum (at most M) adds M u: 9 M u.  bot likewise.  bot - top (at most 2M) inherits
# 18 M u and rounds by 2M u: 20 M u; times ty: + 2M 2u + 2M u = 26 M u; plus top's 9 M u and the last sum's rounding M u: 36 M u.
# Eleven roundings, each weighed by the largest magnitude it can act on; second-order terms are below 1e-6 of this.
LINEAR_F32_ROUNDINGS = 36


def linear_f32_bound(d, clip):
    c = ref.clip(d, clip)
    m = float(np.abs(c[np.isfinite(c)]).max(initial=0.0))
    return LINEAR_F32_ROUNDINGS * m * 2.0 ** -24 * (1 + 1e-6)


def check_shape(drv, shape, levels_of=ref.levels, depth=True):
    """Every picture of the shape pair through both filters against the restatement.  levels_of: the build's levels of an fp32 frame
    (the GPU build may fuse x * 255 + 0.5: its own sgs_pack_rgba8 says)."""
    W, H, w, h = shape
    label = shape_id(shape)
    check_picture_properties(shape)                        # before the library's output is looked at
    for name, pic in pictures_of(shape).items():
        lv = levels_of(pic)
        assert np.abs(lv.astype(int) - ref.levels(pic).astype(int)).max() <= 1
        want, want_lv = ref.resize_rgb8(pic, w, h, "bicubic", lv)
        got = drv.one(pic, (w, h), "rgb8", "bicubic")
        assert np.array_equal(_bits(got), _bits(want)), \
            f"{label} {name}: bicubic rgb8 differs from the restatement at {int((_bits(got) != _bits(want)).sum())} of {want.size} values " \
            f"(first: {got.reshape(-1)[np.argmax(_bits(got).reshape(-1) != _bits(want).reshape(-1))] * 255:.3f} for level {want_lv.reshape(-1)[np.argmax(_bits(got).reshape(-1) != _bits(want).reshape(-1))]})"
        want, _ = ref.resize_rgb8(pic, w, h, "linear", lv)
        got = drv.one(pic, (w, h), "rgb8", "linear")
        assert np.array_equal(_bits(got), _bits(want)), f"{label} {name}: linear rgb8 differs from the restatement at {int((_bits(got) != _bits(want)).sum())} of {want.size} values"
    if not depth:
        return
    for name, (d, clip) in depth_pictures(W, H).items():
        want = ref.bicubic_f32(d, w, h, clip)
        got = drv.one(d, (w, h), "f32", "bicubic", clip)
        ok = ~np.isnan(want)                               # (single_nan: the pixels whose windows miss the NaN)
        assert name == "single_nan" or ok.all()
        assert np.array_equal(_bits(got)[ok], _bits(want)[ok]), f"{label} {name}: bicubic f32 differs from the restatement at {int((_bits(got)[ok] != _bits(want)[ok]).sum())} of {int(ok.sum())} values"
        exact = ref.linear_f(d, w, h, clip, dtype=np.float64)
        got = drv.one(d, (w, h), "f32", "linear", clip)
        ok = ~np.isnan(exact)
        bound = linear_f32_bound(d, clip)
        with np.errstate(invalid="ignore"):
            err = float(np.abs(got.astype(np.float64) - exact)[ok].max()) if ok.any() else 0.0
        print(f"[resize] {label} {name}: linear f32 within {err:.3e} of the fp64 lerps (bound {bound:.3e})")
        assert err <= bound, f"{label} {name}: linear f32 is {err:.3e} from the fp64 lerps (bound {bound:.3e})"


def check_downstream(drv, png, shape, levels_of=ref.levels):
    """pack_rgba8(resize(x)) and the decoded encode_png(resize(x)) are the restatement's levels."""
    W, H, w, h = shape
    for name in ("thresholds", "random"):
        pic = pictures_of(shape)[name]
        for filt in ("bicubic", "linear"):
            _, want_lv = ref.resize_rgb8(pic, w, h, filt, levels_of(pic))
            out = drv.one(pic, (w, h), "rgb8", filt)
            assert np.array_equal(drv.pack(out), want_lv), f"{shape_id(shape)} {name} {filt}: pack_rgba8 of the resized frame shows other levels"
            data = png.encode_one(out, "rgb8")
            got = decode_png_rgb(data, w, h)
            assert np.array_equal(got, want_lv), f"{shape_id(shape)} {name} {filt}: the PNG of the resized frame holds other levels"


def decode_png_rgb(data, w, h):
    """The samples of an 8-bit RGB PNG by tests/png_ref.py's parser and zlib alone."""
    import zlib
    parsed = png_ref.parse_png(data)
    assert parsed["ihdr"] == (w, h, 8, 2, 0, 0, 0), parsed["ihdr"]
    rows = np.frombuffer(zlib.decompress(b"".join(b for t, b in parsed["chunks"] if t == b"IDAT")), np.uint8).reshape(h, 3 * w + 1)
    out = np.zeros((h, 3 * w), np.uint8)
    prev = np.zeros(3 * w, np.int64)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        cur = np.zeros(3 * w, np.int64)
        for i in range(3 * w):
            a = cur[i - 3] if i >= 3 else 0
            b = prev[i]
            c = prev[i - 3] if i >= 3 else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (line[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3)


def check_batch_and_strides(drv, shape=(37, 23, 13, 7)):
    """Three frames with padded source and destination strides equal the frames resized alone, bit for bit; dst's padding is untouched."""
    W, H, w, h = shape
    pics = pictures_of(shape)
    frames = np.stack([pics["random"], pics["checker"], pics["thresholds"]])
    depth = np.stack([depth_pictures(W, H)["plateaus"][0] * np.float32(s) for s in (1.0, 0.5, 0.25)])
    for fmt, fr, ch in (("rgb8", frames, 3), ("f32", depth, 1)):
        for filt in ("bicubic", "linear"):
            r = drv.resize(fr, (w, h), fmt, filt, src_stride=H * W * ch + 37, dst_stride=h * w * ch + 11)
            check_padding_untouched(r)
            for i in range(3):
                alone = drv.one(fr[i], (w, h), fmt, filt)
                assert np.array_equal(_bits(r["out"][i]), _bits(alone)), f"{fmt} {filt}: frame {i} depends on the batch it is issued in"
            packed = drv.resize(fr, (w, h), fmt, filt)
            check_padding_untouched(packed)
            assert np.array_equal(_bits(packed["out"]), _bits(r["out"]))


def check_refusals(drv):
    """Every invalid argument returns SGS_ERR_INVALID with a message and leaves dst untouched; n_frames == 0 is SGS_OK."""
    capi, lib, ctx = drv._capi, drv.lib, drv.ctx
    src = np.zeros(2 * 8 * 8 * 3 + 64, np.float32)
    keep_s, s_ptr = drv._frames(src)
    keep_d, d_ptr, d_get = drv._floats(np.full(4096, SENTINEL, np.float32))
    nan, inf = float("nan"), float("inf")

    def call(w=8, h=8, n=2, fmt=capi.RESIZE_RGB8, filt=capi.RESIZE_BICUBIC, dw=4, dh=4, lo=-inf, hi=inf, reserved=(0, 0), s=s_ptr, d=d_ptr,
             params=True, ss=192, ds=48):
        p = capi.SgsResizeParams(fmt, filt, dw, dh, lo, hi, (C.c_int32 * 2)(*reserved))
        return drv.call(s, w, h, n, ss, p if params else None, d, ds)

    bad = [(b"format 2 ", dict(fmt=2)), (b"format -1 ", dict(fmt=-1)), (b"filter 2 ", dict(filt=2)), (b"filter -1 ", dict(filt=-1)),
           (b"reserved = {7, 0}", dict(reserved=(7, 0))), (b"reserved = {0, 1}", dict(reserved=(0, 1))),
           (b"null src", dict(s=None)), (b"null dst", dict(d=None)), (b"params is NULL", dict(params=False)), (b"n_frames = -1", dict(n=-1)),
           (b"source 0 x 8", dict(w=0)), (b"source 8 x 0", dict(h=0)), (b"source 65536 x 8", dict(w=65536)), (b"source 8 x 65536", dict(h=65536)),
           (b"destination 0 x 4", dict(dw=0)), (b"destination 4 x 0", dict(dh=0)), (b"destination 65536 x 4", dict(dw=65536)),
           (b"destination 4 x 65536", dict(dh=65536)), (b"destination -3 x 4", dict(dw=-3)),
           (b"src frames overlap", dict(ss=191)), (b"dst frames overlap", dict(ds=47)),
           (b"src frames overlap", dict(fmt=capi.RESIZE_F32, ss=63, ds=16)), (b"dst frames overlap", dict(fmt=capi.RESIZE_F32, ss=64, ds=15)),
           (b"clip_lo 2 is above clip_hi 1", dict(lo=2.0, hi=1.0)), (b"clip bound is NaN", dict(lo=nan)), (b"clip bound is NaN", dict(hi=nan)),
           (b"src and dst overlap", dict(d=s_ptr)), (b"src and dst overlap", dict(d=s_ptr + 4 * (192 + 191), n=2)),
           (b"src and dst overlap", dict(s=d_ptr + 4 * 47, n=1))]
    for word, kw in bad:
        assert call(**kw) == -1, word
        assert word in lib.sgs_last_error(ctx), (word, lib.sgs_last_error(ctx))
    drv._sync()
    assert (np.array(d_get()) == SENTINEL).all(), "a refused call wrote to dst"
    # n_frames == 0 launches nothing, null buffers or not; a refused parameter is refused all the same
    assert call(n=0) == 0 and call(n=0, s=None, d=None) == 0 and call(n=0, fmt=9) == -1
    drv._sync()
    assert (np.array(d_get()) == SENTINEL).all()
    # buffers that touch without overlapping, and the limits themselves, are accepted
    assert call(s=d_ptr + 4 * 48, n=1) == 0
    assert call(lo=1.0, hi=1.0, fmt=capi.RESIZE_F32, ss=64, ds=16) == 0
    d = capi.SgsResizeParams()
    lib.sgs_resize_params_default(C.byref(d))
    assert (d.format, d.filter, d.dst_width, d.dst_height, d.clip_lo, d.clip_hi, tuple(d.reserved)) == (0, 0, 320, 240, -inf, inf, (0, 0))
    for bad_name in (dict(format="rgba8"), dict(filter="lanczos")):
        try:
            capi.resize_params(**bad_name)
        except ValueError:
            continue
        raise AssertionError(f"resize_params accepted {bad_name}")
