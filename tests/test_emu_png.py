"""The PNG encoder (sgs_encode_png, csrc/sgs_png.h) under the wave64 emulator: the kernels' own source, on the CPU.

On every picture: 1 lossless (PIL reads the restated samples), 2 structure (chunk list, IHDR, CRCs, the zlib stream and its Adler-32,
every strip inflating alone), 3 the filter of every row, 4 sizes, 5 against zlib on the same strips with run matches only.  Once each:
6 issue independence, 7 capacity, 11 refusals.  The figures are printed (pytest -s) and listed in DESIGN.md §12."""
import ctypes as C

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


COLOUR = pc.colour_set()
DEPTH = pc.depth_set()


@pytest.mark.parametrize("name", sorted(COLOUR))
def test_colour_files(drv, name):
    """Checks 1-5 (and no byte past the reported size: the sentinel check of encode_one)."""
    img = COLOUR[name]
    h, w = img.shape[:2]
    fig = pc.check_file(drv.encode_one(img, "rgb8"), png_ref.rgb_samples(img), drv.bound(w, h, "rgb8"), name)
    pc.check_smaller_than_raw(fig, name, noise=name.startswith("noise"))
    if name == "constant_640x48":
        # a 258-byte match costs at most 13 bits even in fixed codes, plus ~300 bytes of framing and table per strip
        assert fig["bytes"] <= 0.02 * fig["raw"], fig
    if name == "filter_tie_48x32":
        assert fig["tied_rows"] >= 8, "the picture was built to make filters tie"
    if name == "noise_64x64":
        assert fig["bytes"] == fig["bound"], "incompressible input goes the stored path: exactly the bound"


@pytest.mark.parametrize("name", sorted(DEPTH))
def test_depth_files(drv, name):
    img = DEPTH[name]
    h, w = img.shape
    fig = pc.check_file(drv.encode_one(img, "depth16"), png_ref.depth_samples(img), drv.bound(w, h, "depth16"), name)
    pc.check_smaller_than_raw(fig, name)


def test_depth_special_values_and_other_scales(drv):
    """+inf -> depth_max, -inf / NaN / negatives -> 0, values beyond depth_max -> depth_max; another scale and maximum; a product of
    exactly 65535 is accepted and fills the 16 bits."""
    d = np.float32([[np.inf, -np.inf, np.nan, -3.0, 7.0, 6.5, 0.0, 0.00009999, 0.0001, 3.14159]])
    s = png_ref.depth_samples(d)
    assert s.tolist() == [[65000, 0, 0, 0, 65000, 65000, 0, 0, 1, 31415]]
    pc.check_file(drv.encode_one(d, "depth16"), s, drv.bound(10, 1, "depth16"), "depth_special", against_zlib=False)
    s2 = png_ref.depth_samples(d, 1000.0, 10.0)
    pc.check_file(drv.encode_one(d, "depth16", depth_scale=1000.0, depth_max=10.0), s2, drv.bound(10, 1, "depth16", 1000.0, 10.0), "depth_mm", against_zlib=False)
    s3 = png_ref.depth_samples(d * 10000, 1.0, 65535.0)
    assert s3.max() == 65535
    pc.check_file(drv.encode_one(d * 10000, "depth16", depth_scale=1.0, depth_max=65535.0), s3, drv.bound(10, 1, "depth16", 1.0, 65535.0), "depth_full_range", against_zlib=False)


def test_parser_refuses_damage(drv):
    """The checker's own sensitivity: a flipped payload bit, a wrong length, a byte after IEND and a bad signature are refused; a
    flipped bit with a repaired CRC fails in zlib (Adler-32 or the code itself)."""
    import struct
    import zlib
    good = drv.encode_one(COLOUR["colour_17x33"], "rgb8")
    png_ref.parse_png(good)
    at = good.index(b"IDAT") + 40
    flipped = good[:at] + bytes([good[at] ^ 4]) + good[at + 1:]
    for bad in (flipped, good[:8] + b"\x00\x00\x00\x0e" + good[12:], good + b"\x00", b"\x88" + good[1:], good[:-1]):
        with pytest.raises(png_ref.PngError):
            png_ref.parse_png(bad)
    i = good.index(b"IDAT")
    n, = struct.unpack(">I", good[i - 4:i])
    body = flipped[i + 4:i + 4 + n]
    with pytest.raises(zlib.error):
        zlib.decompress(body)


def test_issue_independence(drv):
    """Test 6: a batch of 5 different 250x187 frames yields the bytes each yields alone; two calls yield the same bytes; a permuted
    batch yields permuted files.  Colour and depth."""
    frames = np.stack([jpeg_cases.gradient_noise(187, 250, seed=s) * (0.5 + 0.1 * s) for s in range(5)])
    for fmt, fr in (("rgb8", frames), ("depth16", np.ascontiguousarray(frames[..., 0] * 7.0))):
        batch = drv.encode(fr, fmt)
        assert batch["rc"] == 0
        jpeg_cases.check_nothing_written_beyond(batch)
        assert drv.encode(fr, fmt)["files"] == batch["files"]
        assert len(set(batch["files"])) == 5
        for i in range(5):
            assert drv.encode_one(fr[i], fmt) == batch["files"][i], f"frame {i} depends on the batch it is issued in"
        perm = [3, 1, 4, 0, 2]
        assert drv.encode(fr[perm], fmt)["files"] == [batch["files"][k] for k in perm]


def test_capacity(drv):
    """Test 7: one byte short — the status says overflow, the sizes are unchanged, earlier frames are byte-identical and nothing is
    written beyond the last frame that fits; with exactly the bytes needed the call succeeds."""
    frames = np.stack([jpeg_cases.gradient_noise(40, 56, seed=s) for s in range(3)])
    full = drv.encode(frames, "rgb8")
    assert full["rc"] == 0
    need = full["needed"]
    short = drv.encode(frames, "rgb8", capacity=need - 1)
    assert short["rc"] == -4 and short["needed"] == need, (short["rc"], short["needed"])        # SGS_ERR_OVERFLOW
    assert b"out_capacity" in drv.lib.sgs_last_error(drv.ctx)
    assert (short["sizes"] == full["sizes"]).all() and (short["offsets"] == full["offsets"]).all()
    jpeg_cases.check_nothing_written_beyond(short)
    cut = int(full["offsets"][2])
    assert bytes(short["buffer"][:cut]) == bytes(full["buffer"][:cut]) and (short["buffer"][cut:] == pc.SENTINEL).all()
    none = drv.encode(frames, "rgb8", capacity=0)
    assert none["rc"] == -4 and (none["buffer"] == pc.SENTINEL).all() and (none["sizes"] == full["sizes"]).all()
    exact = drv.encode(frames, "rgb8", capacity=need)
    assert exact["rc"] == 0 and exact["files"] == full["files"]
    assert need <= 3 * drv.bound(56, 40, "rgb8")


def test_bound_is_the_stored_size(drv):
    """sgs_png_bound is derived: 56 bytes around the strips, 22 per strip, the filtered bytes."""
    assert drv.bound(1, 1, "rgb8") == 56 + 22 + 4
    assert drv.bound(640, 480, "depth16") == 56 + 22 * 40 + 480 * 1281          # 12 rows of 1 281 bytes per strip
    assert drv.bound(1024, 768, "rgb8") == 56 + 22 * 154 + 768 * 3073           # 5 rows of 3 073 bytes per strip
    assert drv.bound(5461, 2, "rgb8") == 56 + 22 * 2 + 2 * 16384


def test_refusals(drv):
    """Test 11: every invalid argument returns SGS_ERR_INVALID with a message of its own and leaves `out` untouched."""
    lib, ctx = drv.lib, drv.ctx
    f = np.zeros((2, 8, 8, 3), np.float32)
    wide = np.zeros(3 * 8192, np.float32)
    out = np.full(1 << 16, pc.SENTINEL, np.uint8); offs = np.zeros(2, np.int64); sizes = np.zeros(2, np.int64)
    one_up = float(np.nextafter(np.float32(65535.0), np.float32(1e9)))

    def call(w=8, h=8, n=2, fmt=_capi.PNG_RGB8, scale=10000.0, dmax=6.5, reserved=0, src=f.ctypes.data, o=out.ctypes.data, a=offs.ctypes.data,
             s=sizes.ctypes.data, params=True, cap=out.size, stride=192):
        p = _capi.SgsPngParams(fmt, scale, dmax, reserved)
        return lib.sgs_encode_png(ctx, src, w, h, n, stride, C.byref(p) if params else None, o, cap, a, s, None)

    assert call() == 0 and lib.sgs_png_status(ctx, None) == 0
    out[:] = pc.SENTINEL
    D = _capi.PNG_DEPTH16
    bad = [(b"format 2 ", dict(fmt=2)), (b"format -1 ", dict(fmt=-1)), (b"reserved = 7", dict(reserved=7)),
           (b"null src", dict(src=None)), (b"null out", dict(o=None)), (b"null out_offsets", dict(a=None)), (b"null out_sizes", dict(s=None)),
           (b"params is NULL", dict(params=False)), (b"n_frames = -1", dict(n=-1)), (b"capacity -1", dict(cap=-1)),
           (b"0 x 8", dict(w=0)), (b"8 x 0", dict(h=0)), (b"8 x 65536", dict(h=65536)),
           (b"width 5462", dict(w=5462, h=1, n=1, src=wide.ctypes.data)), (b"width 8192", dict(w=8192, h=1, n=1, fmt=D, src=wide.ctypes.data)),
           (b"depth_scale 0 ", dict(fmt=D, scale=0.0)), (b"depth_scale -1 ", dict(fmt=D, scale=-1.0)), (b"depth_max 0 ", dict(fmt=D, dmax=0.0)),
           (b"does not fit 16 bits", dict(fmt=D, scale=1.0, dmax=one_up)), (b"does not fit 16 bits", dict(fmt=D, scale=10000.0, dmax=6.6)),
           (b"frames overlap", dict(stride=191)), (b"frames overlap", dict(fmt=D, stride=63))]
    for word, kw in bad:
        assert call(**kw) == -1, word
        assert word in lib.sgs_last_error(ctx), (word, lib.sgs_last_error(ctx))
    assert (out == pc.SENTINEL).all(), "a refused call wrote to out"
    # the limits themselves are accepted
    assert call(w=5461, h=1, n=1, src=wide.ctypes.data) == 0 and call(w=8191, h=1, n=1, fmt=D, src=wide.ctypes.data) == 0
    assert call(fmt=D, scale=1.0, dmax=65535.0, stride=64) == 0
    # a call that encodes nothing clears the status of the one before it
    assert call(cap=10) == 0 and lib.sgs_png_status(ctx, None) == -4
    assert call(n=0) == 0 and lib.sgs_png_status(ctx, None) == 0
    d = _capi.SgsPngParams()
    lib.sgs_png_params_default(C.byref(d))
    assert (d.format, d.depth_scale, d.depth_max, d.reserved) == (_capi.PNG_RGB8, 10000.0, 6.5, 0)
    assert lib.sgs_png_bound(0, 8, C.byref(d)) == -1 and lib.sgs_png_bound(8, 65536, C.byref(d)) == -1 and lib.sgs_png_bound(5462, 1, C.byref(d)) == -1
    assert lib.sgs_png_bound(8, 8, None) == -1
    with pytest.raises(ValueError):
        _capi.png_params("rgba8")
