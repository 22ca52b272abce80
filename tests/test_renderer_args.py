"""The frame operators' argument checks in sage_gs/renderer.py (_frames_arg, _frame_stride, _out_arg, _maps_arg, _rows_arg), on CPU
tensors: the device is an argument, a "meta" tensor stands for one on another device, and no library is loaded.  Frames of 2 x 3
pixels, batches of 0, 1 and 3."""
import numpy as np
import pytest
import torch

from sage_gs.renderer import _frame_stride, _frames_arg, _maps_arg, _out_arg, _rows_arg

CPU = torch.device("cpu")
H, W = 2, 3
RGB, GREY = (None, None, 3), (None, None)


def _refused(call, *args, starts=None, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    assert starts is None or str(e.value).startswith(starts), str(e.value)


def test_frames_arg_takes_a_frame_or_a_batch():
    one = torch.rand(H, W, 3)
    frames, single = _frames_arg(one, CPU, torch.float32, RGB, "rgb")
    assert single and tuple(frames.shape) == (1, H, W, 3) and frames.data_ptr() == one.data_ptr()
    batch = torch.rand(3, H, W, 3)
    frames, single = _frames_arg(batch, CPU, torch.float32, RGB, "rgb")
    assert not single and frames is batch
    grey, single = _frames_arg(torch.zeros(H, W, dtype=torch.int32), CPU, torch.int32, GREY, "ids", 1)
    assert single and tuple(grey.shape) == (1, H, W)
    big = torch.rand(6, H, W, 3)
    cut = big[::2]                                                   # a strided batch of contiguous frames
    frames, single = _frames_arg(cut, CPU, torch.float32, RGB, "rgb")
    assert not single and frames is cut and frames.stride(0) == 2 * H * W * 3


def test_frames_arg_refusals():
    big = torch.rand(3, H, 2 * W, 3)
    for bad in (big[:, :, ::2],                                      # frames that are not contiguous
                torch.rand(3, H, W, 3, dtype=torch.float64),         # dtype
                torch.rand(3, H, W, 4), torch.rand(H, W, 4),         # tail
                torch.rand(W, 3), torch.rand(2, 3, H, W, 3),         # rank
                np.zeros((H, W, 3), np.float32), None,               # not a tensor
                torch.empty(3, H, W, 3, device="meta")):             # another device
        _refused(_frames_arg, bad, CPU, torch.float32, RGB, "rgb", starts="rgb must be float32 [H,W,3] or [B,H,W,3]")
    _refused(_frames_arg, torch.rand(3, H, W, 3), CPU, torch.float32, GREY, "depth", 1, starts="depth must be float32 [H,W] or [B,H,W]")
    none = torch.rand(0, H, W, 3)
    frames, single = _frames_arg(none, CPU, torch.float32, RGB, "rgb", 0)
    assert not single and frames.shape[0] == 0
    _refused(_frames_arg, none, CPU, torch.float32, RGB, "rgb", 1)
    empty = torch.rand(3, 0, W, 3)                                   # frames without a pixel: the library's to refuse where no frame is
    assert _frames_arg(empty, CPU, torch.float32, RGB, "rgb", 0)[0] is empty                       # asked for, refused here where one is
    _refused(_frames_arg, empty, CPU, torch.float32, RGB, "rgb", 1)


def test_frame_stride():
    big = torch.rand(6, H, W, 3)
    size = H * W * 3
    assert _frame_stride(big, size) == size and _frame_stride(big[::2], size) == 2 * size
    one = big[::2][:1]
    assert one.stride(0) == 2 * size and _frame_stride(one, size) == size        # one frame: its element count, whatever the view says
    assert _frame_stride(big[:0], size) == size


def test_out_arg():
    got = _out_arg(None, CPU, (3, H, W), torch.int32, "out", zero=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, H, W) and got.device == CPU and not got.any()
    got = _out_arg(None, CPU, [H, W], torch.float32, "out")
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
    mine = torch.full((3, H, W), 7, dtype=torch.int32)
    assert _out_arg(mine, CPU, (3, H, W), torch.int32, "out[0]") is mine and (mine == 7).all()
    for bad in (torch.zeros(3, H, W + 1, dtype=torch.int32), torch.zeros(3, H, W), torch.zeros(3, H, 2 * W, dtype=torch.int32)[:, :, ::2],
                torch.empty(3, H, W, dtype=torch.int32, device="meta")):
        _refused(_out_arg, bad, CPU, (3, H, W), torch.int32, "out[0]", starts="out[0] must be a contiguous int32 [3, 2, 3] tensor")
    _refused(_out_arg, mine, CPU, (3, H, W), torch.float32, "out_depth", starts="out_depth must be")


def test_maps_arg_layouts():
    mask = torch.rand(H, W) > 0.5
    maps, batched, b, ny, nx, stride = _maps_arg(mask, CPU, torch.uint8, 1, "a mask")
    assert maps.dtype == torch.uint8 and maps.data_ptr() == mask.data_ptr() and tuple(maps.shape) == (1, H, W)
    assert (batched, b, ny, nx, stride) == (False, 1, H, W, H * W)
    d2 = torch.zeros(3, H, W, dtype=torch.int32)
    maps, batched, b, ny, nx, stride = _maps_arg(d2, CPU, torch.int32, 1, "src")
    assert maps is d2 and (batched, b, ny, nx, stride) == (True, 3, H, W, H * W)
    seen = torch.zeros(6, H, W, 2, dtype=torch.int32)
    maps, batched, b, ny, nx, stride = _maps_arg(seen[::2], CPU, torch.int32, 2, "a seen map")
    assert (batched, b, ny, nx, stride) == (True, 3, H, W, 2 * H * W * 2) and tuple(maps.shape) == (3, H, W, 2)
    maps, batched, b, ny, nx, stride = _maps_arg(seen[4], CPU, torch.int32, 2, "a seen map")
    assert (batched, b, ny, nx, stride) == (False, 1, H, W, H * W * 2) and tuple(maps.shape) == (1, H, W, 2)
    assert _maps_arg(seen[::2][:1], CPU, torch.int32, 2, "a seen map")[5] == H * W * 2              # one map: _frame_stride's rule


def test_maps_arg_refusals():
    seen = torch.zeros(3, H, W, 2, dtype=torch.int32)
    _refused(_maps_arg, np.zeros((H, W), np.uint8), CPU, torch.uint8, 1, "a mask", starts="src must be a tensor")
    _refused(_maps_arg, torch.zeros(H, W, dtype=torch.uint8, device="meta"), CPU, torch.uint8, 1, "a mask", starts="src must be a tensor")
    _refused(_maps_arg, torch.zeros(H, W), CPU, torch.uint8, 1, "a mask", starts="a mask must be uint8 or bool [ny,nx] or [B,ny,nx]")
    _refused(_maps_arg, torch.zeros(W, dtype=torch.uint8), CPU, torch.uint8, 1, "a mask", starts="a mask must be")
    _refused(_maps_arg, seen, CPU, torch.int32, 1, "src", starts="src must be int32 [ny,nx] or [B,ny,nx]")
    _refused(_maps_arg, seen[..., :1], CPU, torch.int32, 2, "a seen map", starts="a seen map must be int32 [ny,nx,2] or [B,ny,nx,2]")
    _refused(_maps_arg, torch.zeros(H, W, dtype=torch.bool), CPU, torch.int32, 2, "a seen map", starts="a seen map must be")
    wide = torch.zeros(3, H, 2 * W, dtype=torch.uint8)
    _refused(_maps_arg, wide[:, :, ::2], CPU, torch.uint8, 1, "a mask", starts="src must hold at least one map, each contiguous")
    for shape in ((0, H, W), (3, 0, W), (3, H, 0), (0, W)):
        _refused(_maps_arg, torch.zeros(shape, dtype=torch.uint8), CPU, torch.uint8, 1, "a mask", starts="src must hold at least one map")
    lapped = torch.as_strided(torch.zeros(3 * H * W, dtype=torch.uint8), (3, H, W), (H * W - 1, W, 1))   # maps a cell short of a map apart
    _refused(_maps_arg, lapped, CPU, torch.uint8, 1, "a mask", starts="src must hold at least one map")
    assert _maps_arg(lapped[:1], CPU, torch.uint8, 1, "a mask")[5] == H * W


def test_rows_arg():
    rows = [[0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.5]]
    for given in (rows, np.array(rows, np.float32), torch.tensor(rows, dtype=torch.float32), torch.tensor(rows, dtype=torch.float64)):
        got = _rows_arg(given, CPU, torch.float64, 4, "segments")
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 4) and got.is_contiguous() and got.tolist() == rows
    q = [[0, 1, 2], [1, 0, 0], [2, 5, 4]]
    for given in (q, np.array(q, np.int64), torch.tensor(q, dtype=torch.int64), torch.tensor(q, dtype=torch.int64).t().contiguous().t()):
        got = _rows_arg(given, CPU, torch.int32, 3, "queries")
        assert got.dtype == torch.int32 and tuple(got.shape) == (3, 3) and got.is_contiguous() and got.tolist() == q
    for bad in ([], np.zeros((0, 4)), torch.zeros(0, 4), [[0.0, 1.0, 2.0]], np.zeros((2, 5)), [0.0, 1.0, 2.0, 3.0], np.zeros((1, 2, 4))):
        _refused(_rows_arg, bad, CPU, torch.float64, 4, "segments", starts="segments must be [n,4] with n >= 1")
    for big in (2 ** 31, -2 ** 31 - 1, 2 ** 40):
        _refused(_rows_arg, [[0, 1, big]], CPU, torch.int32, 3, "queries", starts="queries must hold int32 values")
    assert _rows_arg([[0, 1, 2 ** 31 - 1]], CPU, torch.int32, 3, "queries").tolist() == [[0, 1, 2 ** 31 - 1]]
