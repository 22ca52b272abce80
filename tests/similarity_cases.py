"""The image similarity's checks (sgs_image_similarity), shared by the CPU-emulator tests (test_emu_similarity.py, its mutants) and the
GPU tests (test_gpu_similarity.py): the shapes and pictures, a driver of the C ABI over plain buffers, and the assertions against
tests/similarity_ref.py.  Every comparison is exact equality of every field of the 64-byte row."""
from __future__ import annotations

import os
import re

import numpy as np

import jpeg_cases
import similarity_ref as ref
from abi_driver import SENTINEL, AbiDriver, GpuBuffers

ROW = ref.ROW_DTYPE.itemsize


def _tile():
    """SGS_SIM_TILE_W, SGS_SIM_TILE_H of include/sage_gs.h (the binding restates them)."""
    import emu_harness
    from sage_gs import _capi
    hdr = open(os.path.join(emu_harness.ROOT, "include", "sage_gs.h")).read()
    tw, th = (int(re.search(rf"#define SGS_SIM_TILE_{a} (\d+)", hdr).group(1)) for a in "WH")
    assert (tw, th) == (_capi.SIMILARITY_TILE_W, _capi.SIMILARITY_TILE_H) and _capi.SIMILARITY_WINDOW == ref.WINDOW
    return tw, th


TILE_W, TILE_H = _tile()


def sizes_of(tile):
    """Frame sizes with 1, tile - 1, tile, tile + 1 and 2 tile + 1 windows along an axis."""
    return tuple(n + ref.WINDOW - 1 for n in (1, tile - 1, tile, tile + 1, 2 * tile + 1))


WIDTHS, HEIGHTS = sizes_of(TILE_W), sizes_of(TILE_H)
# (W, H): every width and every height, each with a small and a large partner; 11 x 11 is a single window
SHAPES = ((WIDTHS[0], HEIGHTS[0]), (WIDTHS[1], HEIGHTS[4]), (WIDTHS[2], HEIGHTS[3]), (WIDTHS[3], HEIGHTS[2]), (WIDTHS[4], HEIGHTS[1]),
          (WIDTHS[4], HEIGHTS[4]), (WIDTHS[0], HEIGHTS[3]), (WIDTHS[3], HEIGHTS[0]))
assert {s[0] for s in SHAPES} == set(WIDTHS) and {s[1] for s in SHAPES} == set(HEIGHTS)


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


# ---- pictures: name -> (frame fp32 [H,W,3], target uint8 [H,W,3]) -----------------------------------------------------------------------
def unlevel(k):
    """The fp32 nearest k / 255: x * 255 + 0.5 takes it back to k, fused or not."""
    return np.asarray(k).astype(np.float32) / np.float32(255.0)


def _smooth(W, H):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([xx / max(W - 1, 1), yy / max(H - 1, 1), 0.5 + 0.5 * np.sin(0.31 * xx + 0.17 * yy)], -1)
    return np.round(255 * img).astype(np.int64)


def pictures_of(shape, seed=0):
    W, H = shape
    rs = np.random.RandomState(1000 * W + H + seed)
    a, b = rs.randint(0, 256, (H, W, 3)), rs.randint(0, 256, (H, W, 3))
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.repeat((255 * ((xx + yy) & 1))[..., None], 3, -1)
    smooth = _smooth(W, H)
    wild = rs.uniform(-0.5, 1.5, (H, W, 3)).astype(np.float32)                       # below 0, above 1, and off the levels in between
    wild[::2, ::3] = unlevel(a[::2, ::3])
    u8 = lambda v: np.ascontiguousarray(v, np.uint8)
    return {
        "identical": (unlevel(a), u8(a)),
        "noise_pair": (unlevel(a), u8(b)),
        "inverse": (unlevel(a), u8(255 - a)),
        "zero_against_255": (np.zeros((H, W, 3), np.float32), np.full((H, W, 3), 255, np.uint8)),
        "checker_against_its_shift": (unlevel(checker), u8(np.roll(checker, 1, 1))),
        "smooth_plus_noise": (unlevel(smooth), u8(np.clip(smooth + rs.randint(-20, 21, (H, W, 3)), 0, 255))),
        "out_of_range": (wild, u8(b)),
    }


# ---- the C ABI over plain buffers ---------------------------------------------------------------------------------------------------------
class AbiSimilarity(AbiDriver):
    """sgs_image_similarity (and sgs_pack_rgba8) over host buffers; a GPU driver overrides the buffer hooks (GpuSimilarity)."""

    def _u8(self, a):
        a = np.ascontiguousarray(a, np.uint8)
        return a, a.ctypes.data

    def call(self, rgb_ptr, W, H, n, rgb_stride, tgt_ptr, tgt_stride, rows_ptr, stream=None):
        return int(self.lib.sgs_image_similarity(self.ctx, rgb_ptr, int(W), int(H), int(n), int(rgb_stride), tgt_ptr, int(tgt_stride), rows_ptr, stream))

    def rows(self, frames, targets, rgb_stride=None, target_stride=None, slack=64, stream=None):
        """frames fp32 [n,H,W,3]; targets uint8 [n,H,W,3], or [H,W,3]: one target for every frame (target_frame_stride 0) -> ROW_DTYPE [n].
        out_rows holds 0xA5 bytes before the call, with `slack` bytes behind it that must stay so.  rgb_stride (floats): the floats
        between frames are NaN and 1e30 in turn; target_stride (bytes): the bytes between targets are 0x5A.  Behind a shared target lie
        n - 1 other pictures (its inverse), which a call that honours the stride of 0 never reads."""
        frames, targets = np.asarray(frames, np.float32), np.asarray(targets, np.uint8)
        n, H, W = frames.shape[:3]
        size = 3 * H * W
        shared = targets.ndim == 3
        fs = size if rgb_stride is None else int(rgb_stride)
        keep_f, f_ptr = self._frames(jpeg_cases.strided(frames, fs))
        if shared:
            assert target_stride is None
            tbuf = np.concatenate([targets.reshape(-1)] + [255 - targets.reshape(-1)] * (n - 1))
            ts = 0
        else:
            ts = size if target_stride is None else int(target_stride)
            tbuf = np.full((n, ts), 0x5A, np.uint8)
            tbuf[:, :size] = targets.reshape(n, size)
        keep_t, t_ptr = self._u8(tbuf.reshape(-1))
        keep_r, r_ptr, r_get = self._bytes(n * ROW + slack)
        self.lib.check(self.call(f_ptr, W, H, n, fs, t_ptr, ts, r_ptr, stream), self.ctx)
        self._sync()
        rb = np.array(r_get())
        assert (rb[n * ROW:] == SENTINEL).all(), "bytes were written behind out_rows"
        return rb[:n * ROW].view(ref.ROW_DTYPE)

    def pack(self, frame):
        """sgs_pack_rgba8 of an fp32 [h,w,3] frame: uint8 [h,w,3] — the build's own levels."""
        h, w = frame.shape[:2]
        keep_f, f_ptr = self._frames(frame)
        keep_o, o_ptr, o_get = self._bytes(h * w * 4)
        self.lib.check(self.lib.sgs_pack_rgba8(self.ctx, f_ptr, o_ptr, w, h, None), self.ctx)
        self._sync()
        rgba = np.array(o_get()).reshape(h, w, 4)
        assert (rgba[..., 3] == 255).all()
        return rgba[..., :3]


class GpuSimilarity(GpuBuffers, AbiSimilarity):
    """AbiSimilarity over torch device buffers, on a Renderer's context."""

    def _u8(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(self.r.device)
        return t, t.data_ptr()


def check_row(name, got, x_levels, target):
    """One frame's row against the restatement; the assertion names the picture and the field."""
    want = ref.row(x_levels, target)
    words = np.frombuffer(np.asarray(got).tobytes(), np.uint8)
    assert not (words.reshape(8, 8) == SENTINEL).all(1).any(), f"{name}: the row was not written whole (0xA5 bytes are left in it)"
    d = ref.first_difference(got, want)
    assert d is None, f"{name}: {d[0]} is {d[1]}, the restatement has {d[2]}"
    assert np.asarray(got).tobytes() == want.tobytes()


def check_picture_properties(shape):
    """What the pictures are built for, from the restatement alone (before the library's output is looked at)."""
    pics = pictures_of(shape)
    W, H = shape
    nw = (W - 10) * (H - 10)
    r = ref.row(ref.levels(pics["identical"][0]), pics["identical"][1])
    assert r["ssim_q"].tolist() == [nw * ref.ONE] * 3 and r["sse"].tolist() == [0, 0, 0] and r["n_windows"] == nw and r["n_pixels"] == W * H
    r = ref.row(ref.levels(pics["zero_against_255"][0]), pics["zero_against_255"][1])
    assert r["sse"].tolist() == [65025 * W * H] * 3
    r = ref.row(ref.levels(pics["inverse"][0]), pics["inverse"][1])
    assert (r["ssim_q"] < 0).all()
    wild = pics["out_of_range"][0]
    assert (wild < 0).any() and (wild > 1).any()
    for name in ("identical", "noise_pair", "inverse", "checker_against_its_shift", "smooth_plus_noise"):
        f = pics[name][0]
        assert np.array_equal(unlevel(ref.levels(f)), f), name                      # on the levels: fusing x * 255 + 0.5 changes nothing


def check_shape(drv, shape, levels_of=ref.levels):
    """Every picture of the shape against the restatement.  levels_of: the build's levels of an fp32 frame (the GPU build may fuse
    x * 255 + 0.5: its own sgs_pack_rgba8 says)."""
    check_picture_properties(shape)
    for name, (frame, target) in pictures_of(shape).items():
        lv = levels_of(frame)
        assert np.abs(lv.astype(int) - ref.levels(frame).astype(int)).max() <= 1
        got = drv.rows(frame[None], target[None])
        check_row(f"{shape_id(shape)} {name}", got[0], lv, target)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
BATCH_SHAPE = (WIDTHS[3], HEIGHTS[1])          # two tiles across, one down


def batch_pictures():
    """Nine different frames and nine different targets of BATCH_SHAPE."""
    W, H = BATCH_SHAPE
    rs = np.random.RandomState(21)
    smooth = _smooth(W, H)
    frames, targets = [], []
    for k in range(9):
        kind = k % 3
        if kind == 0:                                                                # noise on the levels against other noise
            frames.append(unlevel(rs.randint(0, 256, (H, W, 3)))); targets.append(rs.randint(0, 256, (H, W, 3)))
        elif kind == 1:                                                              # a smooth picture against itself plus noise
            pic = np.roll(smooth, 5 * k, 1)
            frames.append(unlevel(pic)); targets.append(np.clip(pic + rs.randint(-20, 21, (H, W, 3)), 0, 255))
        else:                                                                        # out of range and off the levels
            frames.append(rs.uniform(-0.5, 1.5, (H, W, 3)).astype(np.float32)); targets.append(rs.randint(0, 256, (H, W, 3)))
    frames, targets = np.stack(frames).astype(np.float32), np.stack(targets).astype(np.uint8)
    assert len({f.tobytes() for f in frames}) == 9 and len({t.tobytes() for t in targets}) == 9
    return frames, targets


def check_batches(drv, levels_of=ref.levels):
    """B = 1, 3 and 9 frames with padded strides, against per-frame targets and against one shared target: each frame's row is the
    restatement's, and so that of the frame alone."""
    frames, targets = batch_pictures()
    W, H = BATCH_SHAPE
    size = 3 * W * H
    lv = [levels_of(f) for f in frames]
    for B in (1, 3, 9):
        for sel in (slice(0, B), slice(9 - B, 9)):
            ks = list(range(9)[sel])
            got = drv.rows(frames[sel], targets[sel], rgb_stride=size + 37, target_stride=size + 5)
            for j, k in enumerate(ks):
                check_row(f"B = {B}, per-frame targets: frame {k}", got[j], lv[k], targets[k])
            got = drv.rows(frames[sel], targets[4], rgb_stride=size + 37)
            for j, k in enumerate(ks):
                check_row(f"B = {B}, shared target: frame {k}", got[j], lv[k], targets[4])
    tight = drv.rows(frames, targets)
    for k in range(9):
        check_row(f"B = 9, no padding: frame {k}", tight[k], lv[k], targets[k])


def check_split(drv, chunk):
    """2 * chunk + 3 frames of 11 x 11 in one call (chunk: SGS_SIM_MAX_FRAMES of the library driven): two full launches and a short
    one, each with rgb, target and rows re-based; per-frame targets, then a shared one."""
    n = 2 * chunk + 3
    rs = np.random.RandomState(7)
    x, y = rs.randint(0, 256, (n, 11, 11, 3)), rs.randint(0, 256, (n, 11, 11, 3)).astype(np.uint8)
    got = drv.rows(unlevel(x), y, rgb_stride=363 + 3, target_stride=363 + 1)
    for k in range(n):
        check_row(f"split: frame {k} of {n} (launches of {chunk})", got[k], x[k].astype(np.uint8), y[k])
    got = drv.rows(unlevel(x), y[0])
    for k in range(n):
        check_row(f"split, shared target: frame {k} of {n} (launches of {chunk})", got[k], x[k].astype(np.uint8), y[0])
    return n


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def check_refusals(drv):
    """Every refusal of the header returns SGS_ERR_INVALID with a message that names the argument and leaves the poisoned rows
    untouched; then the context still works."""
    W, H, size = 12, 11, 3 * 12 * 11
    keep_f, f_ptr = drv._frames(np.zeros(2 * size + 64, np.float32))
    keep_t, t_ptr = drv._u8(np.zeros(2 * size + 64, np.uint8))
    keep_r, r_ptr, r_get = drv._bytes(2 * ROW + 64)
    assert f_ptr % 8 == 0 and r_ptr % 8 == 0

    def call(rgb=f_ptr, w=W, h=H, n=2, fs=size, tgt=t_ptr, ts=size, rows=r_ptr):
        return drv.call(rgb, w, h, n, fs, tgt, ts, rows)

    bad = [(b"null rgb", dict(rgb=None)), (b"null target", dict(tgt=None)), (b"null out_rows", dict(rows=None)),
           (b"n_frames = 0", dict(n=0)), (b"n_frames = -2", dict(n=-2)),
           (b"width 10", dict(w=10)), (b"height 10", dict(h=10)), (b"width 0", dict(w=0)), (b"height -11", dict(h=-11)),
           (b"width 65536", dict(w=65536, fs=2 ** 40, ts=0)), (b"height 65536", dict(h=65536, fs=2 ** 40, ts=0)),
           (b"rgb_frame_stride", dict(fs=size - 1)), (b"rgb_frame_stride", dict(n=1, fs=0)), (b"rgb_frame_stride", dict(fs=-size)),
           (b"target_frame_stride", dict(ts=size - 1)), (b"target_frame_stride", dict(ts=1)), (b"target_frame_stride", dict(ts=-size)),
           (b"out_rows", dict(rows=r_ptr + 4)), (b"out_rows", dict(rows=r_ptr + 1)), (b"rgb", dict(rgb=f_ptr + 2)), (b"rgb", dict(rgb=f_ptr + 1))]
    for word, kw in bad:
        assert call(**kw) == -1, f"{word.decode()} with {kw} was accepted"
        msg = drv.lib.sgs_last_error(drv.ctx)
        assert word in msg and b"sgs_image_similarity" in msg, (word, msg)
        if "rows" in kw and kw["rows"] or "rgb" in kw and kw["rgb"]:
            assert b"aligned" in msg, msg
    drv._sync()
    assert (np.array(r_get()) == SENTINEL).all(), "a refused call wrote to out_rows"
    assert call() == 0 and call(ts=0) == 0 and call(rows=r_ptr + 8, rgb=f_ptr + 4, tgt=t_ptr + 1) == 0      # aligned again; any byte address for the target
    drv._sync()
    got = np.array(r_get())[8:8 + 2 * ROW].view(ref.ROW_DTYPE)
    assert got["n_windows"].tolist() == [2, 2] and got["n_pixels"].tolist() == [W * H] * 2 and (got["ssim_q"] == 2 * ref.ONE).all() and (got["sse"] == 0).all()
