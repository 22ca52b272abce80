"""`render(camera, gaussians)` — the Python call surface of the MI355X 3DGS scene renderer.

Host code stays Python on PyTorch-ROCm (device memory, streams); every frame is one call into the
C ABI of ``libsage_gs.so`` (include/sage_gs.h) with raw device pointers.  This module stands where the
reference's Isaac Sim render step stood:

    reference                                             here
    ----------------------------------------------------  ---------------------------------------
    open_stage(usd)  (simple_env.py:219)                   Renderer.upload(gaussians) -> Scene
    cam.set_world_pose(position, orientation) (:1284)      Camera(view=...) / camera.from_isaac_pose
    world.step(render=True)x2 ; cam.get_rgba() (:1368-80)  Renderer.render(camera, scene)
    frame loop (generate_images.py:408-436)                Renderer.render_batch(cameras, scene)

There is no CPU fallback: importing this module needs the built HIP library, rendering needs a GPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi


@dataclass
class Camera:
    """Pinhole camera, +Z forward / +X right / +Y down.  `view` is world->camera (4x4, rigid)."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    view: np.ndarray = field(default_factory=lambda: np.eye(4))

    @property
    def tile_rows(self) -> int:
        return (self.height + 15) // 16

    @property
    def tile_cols(self) -> int:
        return (self.width + 15) // 16


@dataclass
class RenderConfig:
    """Constants of stages S2-S6; defaults are the canonical values."""
    near: float = 0.2
    far: float = 1.0e30
    dilation: float = 0.3
    clamp: float = 1.3
    alpha_min: float = 1.0 / 255.0
    alpha_max: float = 0.99
    t_min: float = 1.0e-4
    background: Sequence[float] = (0.0, 0.0, 0.0)
    sh_degree: int = -1


@dataclass
class TopdownGrid:
    """The grid, the depth range and the two height bands of the top-down seen map (include/sage_gs.h sgs_topdown_params; the
    defaults are sgs_topdown_params_default's): nx x ny cells of cell_size metres, cell (0, 0) cornered at (origin_x, origin_y) in
    map coordinates; a depth sample enters when min_z <= z <= max_z (the reference's depth clip, simple_env.py:1578); a point of
    height h is "free" when free_lo <= h <= free_hi and otherwise "occupied" when occ_lo < h <= occ_hi."""
    nx: int = 256
    ny: int = 256
    origin_x: float = -6.4
    origin_y: float = -6.4
    cell_size: float = 0.05
    min_z: float = 0.1
    max_z: float = 6.5
    free_lo: float = -0.15
    free_hi: float = 0.15
    occ_lo: float = 0.15
    occ_hi: float = 1.5

    def c_params(self, clear: bool = True) -> "_capi.SgsTopdownParams":
        return _capi.SgsTopdownParams(int(self.nx), int(self.ny), float(self.origin_x), float(self.origin_y), float(self.cell_size),
                                      float(self.min_z), float(self.max_z), float(self.free_lo), float(self.free_hi),
                                      float(self.occ_lo), float(self.occ_hi), _capi.TOPDOWN_CLEAR if clear else 0, 0)


@dataclass
class Gaussians:
    """A 3DGS scene with activations applied: linear scales, (w,x,y,z) quaternions,
    opacities in (0,1), SH coefficients [N,(d+1)^2,3].  `model_to_world` is the asset transform of
    Data/template.usda:115-124 (rotateXYZ -90,0,0 for SAGE-3D scenes); it is applied by moving the
    camera into model space, which is exact for rigid transforms."""
    means: torch.Tensor
    scales: torch.Tensor
    quats: torch.Tensor
    opacities: torch.Tensor
    sh: torch.Tensor
    sh_degree: int
    model_to_world: Optional[np.ndarray] = None

    def __len__(self):
        return int(self.means.shape[0])


class Scene:
    """Device-resident, re-laid-out copy of a Gaussians object (wave-chunked float4 rows)."""

    def __init__(self, renderer: "Renderer", handle, n, sh_degree, model_to_world):
        self._r, self.handle, self.n, self.sh_degree = renderer, handle, n, sh_degree
        self.model_to_world = model_to_world            # (validated by Renderer.upload* BEFORE the upload: _check_model_to_world)

    def free(self):
        if self.handle:
            self._r._lib.sgs_scene_free(self._r._ctx, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Mesh:
    """A device-resident triangle mesh for depth rendering (the collision mesh of a scene, include/sage_gs.h sgs_mesh_upload).
    `model_to_world` is the RIGID part of the transform it was uploaded with (any scale / shear is already in the vertices)."""

    def __init__(self, renderer: "Renderer", handle, n_vertices, n_triangles, model_to_world):
        self._r, self.handle, self.n_vertices, self.n_triangles = renderer, handle, n_vertices, n_triangles
        self.model_to_world = model_to_world

    def free(self):
        if self.handle:
            self._r._lib.sgs_mesh_free(self._r._ctx, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _split_model_to_world(m):
    """(rigid 4x4, 3x3 to bake into the vertices) with m[:3,:3] = R @ S, R the rotation nearest to it (polar decomposition).  A rigid m
    gives (m, None) — re-orthonormalised as _check_model_to_world does."""
    m = np.array(m, np.float64, copy=True).reshape(4, 4)
    if not np.allclose(m[3], [0.0, 0.0, 0.0, 1.0], atol=1e-12) or not np.isfinite(m).all():
        raise ValueError("model_to_world must be an affine 4x4 with last row (0, 0, 0, 1)")
    a = m[:3, :3]
    if float(np.abs(a @ a.T - np.eye(3)).max()) <= 1.0e-5 and np.linalg.det(a) > 0:
        return _check_model_to_world(m), None
    u, _, vt = np.linalg.svd(a)
    if np.linalg.det(u @ vt) < 0:
        u[:, -1] = -u[:, -1]
    r = u @ vt
    rigid = np.eye(4)
    rigid[:3, :3], rigid[:3, 3] = r, m[:3, 3]
    return rigid, r.T @ a


def _rigid(views: np.ndarray) -> np.ndarray:
    """[...,4,4] float64 CAMERA poses (world -> camera) -> the same, with every 3x3 that is measurably off orthonormal AFTER the cast to
    fp32 (a view composed or inverted in fp32: torch.linalg.inv of a c2w matrix, poses parsed from 6-digit text) replaced by the nearest
    rotation (polar decomposition).  The C ABI wants the rows orthonormal to 1e-5 (include/sage_gs.h) and says so with an error at
    enqueue time; a Python caller gets the projection instead.  Views already orthonormal to 2e-6 pass through bit for bit, and
    one that is off by more than 1e-3 is not a pose with rounding noise: it is left alone and the library reports it.
    Applied to the camera's pose ONLY, before it is composed with a scene's model_to_world — an asset transform is validated on its own
    (_check_model_to_world): a USD xformOp:scale of 1.0003 is a real scale, not rounding noise, and must not be projected away."""
    v = np.array(views, np.float64, copy=True)
    flat = v.reshape(-1, 4, 4)
    if flat.shape[0] == 1:
        # one pose — once per get_rgba() of the adapter: the same test in scalar arithmetic on the fp32-rounded entries (the small-array
        # NumPy form below costs 15 us of a 0.3-ms call); the rare pose that needs projecting takes the general path
        (a, b, c), (d, e, f), (g, h, i) = flat[0, :3, :3].astype(np.float32).tolist()
        dev = max(abs(a * a + b * b + c * c - 1.0), abs(d * d + e * e + f * f - 1.0), abs(g * g + h * h + i * i - 1.0),
                  abs(a * d + b * e + c * f), abs(a * g + b * h + c * i), abs(d * g + e * h + f * i))
        if not (1.5e-6 < dev < 1.1e-3):              # (clear of both thresholds: the verdict is the loop's)
            return v
    for m in flat:
        r = m[:3, :3].astype(np.float32).astype(np.float64)
        dev = np.abs(r @ r.T - np.eye(3)).max()
        if 2.0e-6 < dev < 1.0e-3:
            u, _, vt = np.linalg.svd(m[:3, :3])
            m[:3, :3] = u @ vt
    return v


def _check_model_to_world(m) -> np.ndarray:
    """A scene's model -> world transform must be RIGID (rotation + translation): the renderer applies it by moving the camera into model
    space, which is exact only then.  Off orthonormal by up to 2e-6 (a rotation written in fp32): accepted as it is.  Up to 1e-5 — what the
    library itself tolerates; a product of two fp32 rotations lands at 1e-6 .. 5e-6 — the 3x3 is replaced by the nearest rotation (polar
    decomposition): rounding noise, not a transform.  Anything more — a scale (a USD xformOp:scale of 1.0003 is a REAL scale: 6e-4), a shear,
    a mirror — raises here, with the fix, instead of being silently re-orthonormalised (round 4) or rejected later by the library's
    per-frame rigidity check with a message about the camera.  Called BEFORE the scene is uploaded: a refusal leaves nothing on the device."""
    m = np.array(m, np.float64, copy=True).reshape(4, 4)
    r = m[:3, :3]
    dev = float(np.abs(r @ r.T - np.eye(3)).max())
    if not (dev <= 1.0e-5) or not np.allclose(m[3], [0.0, 0.0, 0.0, 1.0], atol=1e-12) or np.linalg.det(r) < 0:
        raise ValueError(f"model_to_world is not a rigid transform (its 3x3 is off orthonormal by {dev:.3g}): bake the asset's scale / shear into the "
                         "Gaussians' means and scales (a USD xformOp:scale s multiplies both) and pass the rotation + translation only")
    if dev > 2.0e-6:
        u, _, vt = np.linalg.svd(r)
        m[:3, :3] = u @ vt
    return m


def _as_f32(t: torch.Tensor, device, shape_tail):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t, np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"expected [N,{','.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t


# -- the frame operators' argument checks (DESIGN.md §3 "What the operators check"): the device is an argument, so they run where
# there is no GPU.  Each raises ValueError before any library call; a refusal they cannot say is a plain ValueError in the method.
def _dtype_name(dtype) -> str:
    return str(dtype).split(".")[-1]


def _frames_arg(t, device, dtype, tail, what, min_frames=0):
    """(frames [B, *frame], single) of `t`: a `dtype` tensor on `device` holding one frame [*frame] (single) or a batch [B, *frame].
    `tail` is a frame's shape, None where a size is free.  B >= min_frames, and where a frame is asked for it holds an element.  Each
    frame is contiguous; the batch stride is free (see _frame_stride)."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == device and t.dim() in (len(tail), len(tail) + 1)
    single = ok and t.dim() == len(tail)
    if single:
        t = t.unsqueeze(0)
    if (not ok or any(want is not None and have != want for have, want in zip(t.shape[1:], tail)) or t.shape[0] < min_frames
            or (min_frames > 0 and t.numel() == 0) or (t.shape[0] > 0 and not t[0].is_contiguous())):
        dims = ",".join("HW"[k] if want is None else str(want) for k, want in enumerate(tail))
        raise ValueError(f"{what} must be {_dtype_name(dtype)} [{dims}] or [B,{dims}] on the renderer's device with contiguous frames"
                         + (f", at least {min_frames} of them and none empty" if min_frames else ""))
    return t, single


def _frame_stride(frames, frame_elements: int) -> int:
    """The batch stride the library is given, in elements: stride(0) of a batch, and for ONE frame the frame's element count whatever
    its stride(0) says — a one-frame view cut from a strided batch (big[::2][:1]) carries the batch's stride or any other, and
    sgs_object_table / sgs_topdown_map test the stride even for one frame."""
    return int(frames.stride(0)) if frames.shape[0] > 1 else int(frame_elements)


def _out_arg(out, device, shape, dtype, name, zero=False):
    """`out`, checked: a contiguous `dtype` tensor of `shape` on `device`; None allocates it (zeroed if asked)."""
    if out is None:
        return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=device)
    if out.device != device or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {_dtype_name(dtype)} {list(shape)} tensor on the renderer's device")
    return out


def _maps_arg(src, device, dtype, per_cell, what):
    """(maps, batched, b, ny, nx, stride) of grids [ny,nx] or [B,ny,nx] — with per_cell = 2, [ny,nx,2] or [B,ny,nx,2] — of `dtype` on
    `device`; bool stands for uint8 (a view of the same storage).  At least one map, no side empty, every map contiguous, a batch's
    stride(0) at least a map; `stride` is what the library is given."""
    if not isinstance(src, torch.Tensor) or src.device != device:
        raise ValueError("src must be a tensor on the renderer's device")
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    rank = 2 if per_cell == 1 else 3
    if src.dtype != dtype or src.dim() not in (rank, rank + 1) or (per_cell > 1 and src.shape[-1] != per_cell):
        raise ValueError(f"{what} must be {_dtype_name(dtype)}{' or bool' if dtype == torch.uint8 else ''} "
                         + ("[ny,nx] or [B,ny,nx]" if per_cell == 1 else f"[ny,nx,{per_cell}] or [B,ny,nx,{per_cell}]"))
    batched = src.dim() == rank + 1
    maps = src if batched else src.unsqueeze(0)
    b, ny, nx = int(maps.shape[0]), int(maps.shape[1]), int(maps.shape[2])
    if min(b, ny, nx) < 1 or not maps[0].is_contiguous() or (b > 1 and int(maps.stride(0)) < ny * nx * per_cell):
        raise ValueError("src must hold at least one map, each contiguous")
    return maps, batched, b, ny, nx, _frame_stride(maps, ny * nx * per_cell)


def _flat_i32(x, device, what):
    """`x` — a tensor, or anything np.asarray takes — as a contiguous flat int32 tensor on `device` (uint32 values keep their bits)."""
    if not isinstance(x, torch.Tensor):
        a = np.asarray(x, np.int64).reshape(-1)
        if a.size and (a.min() < -2 ** 31 or a.max() > 0xFFFFFFFF):
            raise ValueError(f"{what} must fit 32 bits")
        x = torch.from_numpy(a.astype(np.uint32).view(np.int32) if a.size and a.max() > 0x7FFFFFFF else a.astype(np.int32))
    if x.dtype != torch.int32 or x.dim() != 1:
        raise ValueError(f"{what} must be a flat int32 tensor")
    return x.to(device).contiguous()


def _rows_arg(x, device, dtype, width, what):
    """`x` — a tensor, or anything np.asarray takes — as a contiguous [n,width] tensor of `dtype` on `device`, n >= 1.  Host integers
    that do not fit `dtype` are refused (a tensor's values are not read)."""
    if not isinstance(x, torch.Tensor):
        a = np.asarray(x, np.float64 if dtype.is_floating_point else np.int64)
        if not dtype.is_floating_point and a.size and np.abs(a).max() > torch.iinfo(dtype).max:
            raise ValueError(f"{what} must hold {_dtype_name(dtype)} values")
        x = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x = x.to(device=device, dtype=dtype).contiguous()
    if x.dim() != 2 or x.shape[1] != width or x.shape[0] < 1:
        raise ValueError(f"{what} must be [n,{width}] with n >= 1")
    return x


class Renderer:
    """One rendering context bound to one GPU (one process per GPU is the intended deployment)."""

    def __init__(self, device=None, record_capacity: Optional[int] = None, lib: Optional[_capi.Lib] = None, *,
                 lanes: Optional[int] = None, group: Optional[int] = None, group_lanes: Optional[int] = None,
                 morton: Optional[bool] = None, fine_tile_pixels: Optional[int] = None, fine_tile_growth: Optional[float] = None):
        """lanes / group / group_lanes / morton / record_capacity / fine_tile_pixels: include/sage_gs.h `sgs_tuning` (None = the library's
        default, what the bench runs).  The library reads nothing from the environment; frames do not depend on any of these, bit for bit —
        except fine_tile_pixels / fine_tile_growth (frames of at most that many pixels are rendered through 8x8-pixel tiles, of a quarter of it
        through 4x4, as long as a split multiplies the frame's records by no more than fine_tile_growth: the same splats reach every pixel,
        the blend's coordinates are relative to another tile origin, so frames agree to fp32 rounding)."""
        self._lib = lib or _capi.Lib()
        if not torch.cuda.is_available():
            raise RuntimeError("sage_gs.Renderer needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise ValueError("device must be a cuda (ROCm) device")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        ctx = C.c_void_p()
        self._lib.check(self._lib.sgs_create(index, _capi.BACKEND_HIP, C.byref(ctx)))
        self._ctx = ctx
        if any(v is not None for v in (record_capacity, lanes, group, group_lanes, morton, fine_tile_pixels, fine_tile_growth)):
            self.set_tuning(lanes=lanes, group=group, group_lanes=group_lanes, morton=morton, record_capacity=record_capacity,
                            fine_tile_pixels=fine_tile_pixels, fine_tile_growth=fine_tile_growth)
        self.last_stats = None

    def tuning(self) -> dict:
        t = _capi.SgsTuning()
        self._lib.check(self._lib.sgs_get_tuning(self._ctx, C.byref(t)), self._ctx)
        return {k: (float if k == "fine_tile_growth" else int)(getattr(t, k)) for k, _ in t._fields_}

    def set_tuning(self, **kw):
        """sgs_set_tuning: any of lanes, group, group_lanes, morton, record_capacity, fine_tile_pixels (the others keep their values); applies to the scenes
        uploaded and the frames issued afterwards."""
        t = _capi.SgsTuning()
        self._lib.check(self._lib.sgs_get_tuning(self._ctx, C.byref(t)), self._ctx)
        for k, v in kw.items():
            if k not in dict(t._fields_):
                raise TypeError(f"unknown tuning field {k!r}")
            if v is not None:
                setattr(t, k, float(v) if k == "fine_tile_growth" else int(v))
        self._lib.check(self._lib.sgs_set_tuning(self._ctx, C.byref(t)), self._ctx)

    # -- scene ------------------------------------------------------------------------------------
    def upload(self, g: Gaussians) -> Scene:
        m2w = None if g.model_to_world is None else _check_model_to_world(g.model_to_world)      # (raises before anything is on the device)
        n = len(g)
        k = (g.sh_degree + 1) ** 2
        with torch.cuda.device(self.device):
            means = _as_f32(g.means, self.device, (3,))
            scales = _as_f32(g.scales, self.device, (3,))
            quats = _as_f32(g.quats, self.device, (4,))
            opac = _as_f32(g.opacities.reshape(n), self.device, ())
            sh = _as_f32(g.sh.reshape(n, k, 3), self.device, (k, 3))
            torch.cuda.synchronize(self.device)
            h = C.c_void_p()
            self._lib.check(self._lib.sgs_scene_upload(self._ctx, n, int(g.sh_degree), means.data_ptr(),
                                                       scales.data_ptr(), quats.data_ptr(), opac.data_ptr(),
                                                       sh.data_ptr(), 1, C.byref(h)), self._ctx)
        return Scene(self, h, n, int(g.sh_degree), m2w)

    def upload_compressed(self, chunks, packed, sh, sh_degree: int, model_to_world=None, sh_decode: Optional[str] = None) -> Scene:
        """A scene from the PlayCanvas compressed.ply payload (ply.read_compressed_payload: chunks float32 [nch,18], packed uint32 [n,4],
        sh uint8 [n, 3 k_rest] or None): copied to the device as it is — 16 B + SH bytes per Gaussian — and dequantised there by the
        layout kernel (sgs_scene_upload_compressed); the 8-bit SH coefficients stay bytes in HBM and are dequantised by the projection
        kernel every frame.  NumPy arrays or tensors; tensors already on this device are used in place.
        sh_decode: how a coefficient byte becomes a float — "bin_centre", "linear255" or "bin_centre_ends" (ply.decode_sh_bytes,
        include/sage_gs.h SGS_SH_DECODE_*).  REQUIRED at degree > 0, no default: the tool the reference delegates the decode to could not be
        inspected offline, so say what the tool that wrote / would decompress your file uses."""
        m2w = None if model_to_world is None else _check_model_to_world(model_to_world)          # (raises before anything is on the device)

        def dev(a, dt):
            if a is None:
                return None
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dtype != dt:
                t = t.view(dt) if t.element_size() == torch.empty((), dtype=dt).element_size() else t.to(dt)
            return t.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            c = dev(chunks, torch.float32)
            p = dev(packed if isinstance(packed, torch.Tensor) else np.ascontiguousarray(packed).view(np.int32), torch.int32)
            b = dev(sh, torch.uint8)
            n, nch = int(p.shape[0]), int(c.shape[0])
            if tuple(c.shape) != (nch, 18) or tuple(p.shape) != (n, 4) or nch != (n + 255) // 256:
                raise ValueError("chunks must be [ceil(n/256), 18] and packed [n, 4]")
            k_rest = (int(sh_degree) + 1) ** 2 - 1
            if (k_rest > 0) != (b is not None) or (b is not None and tuple(b.shape) != (n, 3 * k_rest)):
                raise ValueError(f"sh must be uint8 [n, {3 * k_rest}] at degree {sh_degree} (None at degree 0)")
            if k_rest > 0 and sh_decode is None:
                raise ValueError(f"sh_decode is required for a scene with 8-bit SH coefficients: one of {sorted(_capi.SH_DECODE)} (there is no "
                                 "default: ply.decode_sh_bytes / include/sage_gs.h say why)")
            if sh_decode is not None and sh_decode not in _capi.SH_DECODE:
                raise ValueError(f"sh_decode must be one of {sorted(_capi.SH_DECODE)}")
            z = _capi.SgsCompressedScene(n, nch, int(sh_degree), _capi.SH_DECODE[sh_decode] if sh_decode is not None else 0, c.data_ptr(), p.data_ptr(), b.data_ptr() if b is not None else None)
            torch.cuda.synchronize(self.device)
            h = C.c_void_p()
            self._lib.check(self._lib.sgs_scene_upload_compressed(self._ctx, C.byref(z), 1, C.byref(h)), self._ctx)
        return Scene(self, h, n, int(sh_degree), m2w)

    def _scene_of(self, g):
        if isinstance(g, Scene):
            if g._r is not self:
                raise ValueError("this Scene was uploaded by another Renderer (another context, possibly another GPU); "
                                 "upload the Gaussians with the renderer that draws them")
            if g.handle is None:
                raise ValueError("this Scene has been freed")
            return g
        cached = getattr(g, "_sgs_scene", None)
        if cached is None or cached._r is not self or cached.handle is None:
            cached = self.upload(g)
            g._sgs_scene = cached
        return cached

    # -- camera / config marshalling ---------------------------------------------------------------
    @staticmethod
    def _c_camera(cam: Camera, scene: Scene) -> _capi.SgsCamera:
        view = np.asarray(cam.view.detach().cpu().numpy() if isinstance(cam.view, torch.Tensor) else cam.view,
                          np.float64).reshape(4, 4)
        view = _rigid(view)                       # (the camera's pose alone: see _rigid)
        if scene.model_to_world is not None:
            view = view @ scene.model_to_world.reshape(4, 4)
        return _capi.make_camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                                 view.astype(np.float32).tolist())

    _CAM_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                           ("view", "<f4", (16,))])

    @classmethod
    def _c_cameras(cls, cameras: Sequence[Camera], scene: Scene) -> np.ndarray:
        """The sgs_camera array of a batch, marshalled in one go (a structured array with sgs_camera's layout): per-camera
        ctypes marshalling costs ~30 us, as much as a light band of tile rows takes to render."""
        assert cls._CAM_DTYPE.itemsize == C.sizeof(_capi.SgsCamera)
        b = len(cameras)
        views = np.stack([np.asarray(c.view.detach().cpu().numpy() if isinstance(c.view, torch.Tensor) else c.view,
                                     np.float64).reshape(4, 4) for c in cameras])
        views = _rigid(views)                     # (the cameras' poses alone: see _rigid)
        if scene.model_to_world is not None:
            views = views @ scene.model_to_world.reshape(4, 4)
        arr = np.zeros(b, cls._CAM_DTYPE)
        arr["width"] = [c.width for c in cameras]; arr["height"] = [c.height for c in cameras]
        arr["fx"] = [c.fx for c in cameras]; arr["fy"] = [c.fy for c in cameras]
        arr["cx"] = [c.cx for c in cameras]; arr["cy"] = [c.cy for c in cameras]
        arr["view"] = views.reshape(b, 16).astype(np.float32)
        return arr

    def _c_config(self, cfg: Optional[RenderConfig], flags=0) -> _capi.SgsConfig:
        k = self._lib.default_config()
        if cfg is not None:
            k.near_z, k.far_z, k.dilation, k.clamp = cfg.near, cfg.far, cfg.dilation, cfg.clamp
            k.alpha_min, k.alpha_max, k.t_min = cfg.alpha_min, cfg.alpha_max, cfg.t_min
            for i in range(3):
                k.bg[i] = float(cfg.background[i])
            k.sh_degree = int(cfg.sh_degree)
        k.flags = flags
        return k

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- frames -----------------------------------------------------------------------------------
    def render(self, camera: Camera, gaussians, *, config: Optional[RenderConfig] = None,
               out: Optional[torch.Tensor] = None, out_band: Optional[torch.Tensor] = None,
               tile_rows=None, timing=False, sync=True, full_sort=False, out_aux: Optional[torch.Tensor] = None,
               return_aux=False, pipelined=False, loose_cull=False, interleave=None, chunk_cull=True, stats=False,
               deep_cull=True, fine_tiles=True):
        """One frame -> float32 tensor [H,W,3] on this renderer's device (linear RGB).

        fine_tiles=False (tests, A/B): SGS_FLAG_NO_FINE_TILES — 16x16-pixel tiles whatever the frame's size (by default a frame of at most
        `fine_tile_pixels` pixels, 640x480, goes through 8x8-pixel tiles and one of a quarter of that through 4x4: DESIGN.md §4.8).

        stats=True also counts D_f (records consumed by the composite; SGS_FLAG_STATS) — bookkeeping that costs a sweep ~4 %,
        so it is opt-in; N_v, D and the stage times (timing=True) are always available.

        tile_rows=(r0,r1) renders only that band of 16-pixel tile rows (multi-GPU sharding); other rows
        of `out` are left untouched.  With `out_band` (a [>=band rows, W, 3] slab) only the band is
        stored, at the top of the slab, and the slab is returned.  sync=False enqueues on the current
        stream without waiting (collect with .sync()).  pipelined=True (with sync=False) lets the frame overlap
        with other pipelined frames on the library's internal streams: for sweeps of independent frames; the
        output is complete only after .sync().

        interleave=(stride, phase) renders the tile rows phase, phase+stride, ... of the frame (the balanced way to
        shard one frame over `stride` GPUs) into `out_band`, a COMPACT [>= 16 * owned rows, W, 3] image: owned row k
        (frame tile row k*stride + phase) is stored at pixel rows [16k, 16k+16).  tile_rows then indexes owned rows.

        deep_cull=False (tests, A/B): SGS_FLAG_NO_DEEP — no window of a long-lived tile is culled against its live pixels before it is
        ranked; the frame must not change."""
        scene = self._scene_of(gaussians)
        r0, r1 = (0, -1) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        stride, phase = (1, 0) if interleave is None else (int(interleave[0]), int(interleave[1]))
        if stride > 1:
            if out_band is None or out is not None or return_aux or out_aux is not None:
                raise ValueError("interleave renders into out_band (a compact image of the owned rows) only")
            if not 0 <= phase < stride:
                raise ValueError(f"interleave phase {phase} outside [0, {stride})")
            owned = len(range(phase, camera.tile_rows, stride))
            need = 16 * (owned if r1 < 0 else min(r1, owned))
            if (out_band.device != self.device or out_band.dtype != torch.float32 or not out_band.is_contiguous()
                    or out_band.dim() != 3 or out_band.shape[0] < need or tuple(out_band.shape[1:]) != (camera.width, 3)):
                raise ValueError("out_band must be a contiguous float32 [>= 16 * owned rows, W, 3] tensor on the device")
            ptr, ret = out_band.data_ptr(), out_band
        elif out_band is not None:
            if tile_rows is None:
                raise ValueError("out_band needs tile_rows")
            if r1 < 0 or r1 > camera.tile_rows:      # "to the end", as the C ABI reads it
                r1 = camera.tile_rows
            if not 0 <= r0 <= r1:
                raise ValueError(f"tile_rows {tile_rows} is not a band of the frame's {camera.tile_rows} tile rows")
            y0, y1 = r0 * 16, min(r1 * 16, camera.height)
            if (out_band.device != self.device or out_band.dtype != torch.float32 or not out_band.is_contiguous()
                    or out_band.dim() != 3 or out_band.shape[0] < y1 - y0
                    or tuple(out_band.shape[1:]) != (camera.width, 3)):
                raise ValueError("out_band must be a contiguous float32 [>=band rows, W, 3] tensor on the device")
            # the ABI takes the address of pixel (0,0); only the band's rows are ever dereferenced
            ptr, ret = out_band.data_ptr() - y0 * camera.width * 3 * 4, out_band
        else:
            if out is None:
                out = torch.zeros((camera.height, camera.width, 3), dtype=torch.float32, device=self.device)
            elif (out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous()
                  or tuple(out.shape) != (camera.height, camera.width, 3)):
                raise ValueError("out must be a contiguous float32 [H,W,3] tensor on the renderer's device")
            ptr, ret = out.data_ptr(), out
        flags = (0 if sync else _capi.FLAG_ASYNC) | (_capi.FLAG_TIMING if timing else 0) | \
                (_capi.FLAG_FULL_SORT if full_sort else 0) | \
                (_capi.FLAG_LOOSE_CULL if loose_cull else 0) | \
                (0 if chunk_cull else _capi.FLAG_NO_CHUNK_CULL) | (_capi.FLAG_STATS if stats else 0) | \
                (0 if deep_cull else _capi.FLAG_NO_DEEP) | (0 if fine_tiles else _capi.FLAG_NO_FINE_TILES) | \
                (_capi.FLAG_PIPELINED if (pipelined and not sync) else 0)   # full_sort: test hook, orders every queue completely
        cam, cfg, st = self._c_camera(camera, scene), self._c_config(config, flags), _capi.SgsStats()
        cfg.tile_row_stride, cfg.tile_row_phase = stride, phase
        if return_aux or out_aux is not None:
            # f-4: [H,W,2] = expected view depth sum(T alpha z), coverage 1 - T_final (full-frame buffers only)
            if out_band is not None:
                raise ValueError("aux output is not available together with out_band")
            if out_aux is None:
                out_aux = torch.zeros((camera.height, camera.width, 2), dtype=torch.float32, device=self.device)
            self._lib.check(self._lib.sgs_render_rgbd(self._ctx, scene.handle, C.byref(cam), C.byref(cfg), r0, r1, ptr,
                                                      out_aux.data_ptr(), C.byref(st), self._stream()), self._ctx)
            self.last_stats = st.as_dict() if sync else None
            return ret, out_aux
        self._lib.check(self._lib.sgs_render(self._ctx, scene.handle, C.byref(cam), C.byref(cfg), r0, r1,
                                             ptr, C.byref(st), self._stream()), self._ctx)
        self.last_stats = st.as_dict() if sync else None
        return ret

    def sync(self):
        """Complete frames issued with sync=False; returns the statistics of the last one."""
        st = _capi.SgsStats()
        self._lib.check(self._lib.sgs_frame_sync(self._ctx, C.byref(st)), self._ctx)
        self.last_stats = st.as_dict()
        return self.last_stats

    def row_records(self, n_rows: int, reset: bool = True) -> np.ndarray:
        """Records queued per frame tile row, summed over the frames rendered since the last reset (int64 [n_rows]):
        the per-row cost that cost-balanced tile-row bands are cut from (sage_gs.dist).  Covers completed frames (call after sync())."""
        out = np.zeros(int(n_rows), np.int64)
        self._lib.check(self._lib.sgs_row_records(self._ctx, out.ctypes.data, int(n_rows), 1 if reset else 0), self._ctx)
        return out

    def render_batch(self, cameras: Sequence[Camera], gaussians, *, config: Optional[RenderConfig] = None,
                     out: Optional[torch.Tensor] = None, tile_rows=None, want_stats=False, stats=False,
                     out_bands: Optional[torch.Tensor] = None, interleave=None, fine_tiles=True):
        """B frames of one scene in ONE call into the library (camera-sweep batch): the frames go through the pipelined
        lanes, and the per-frame host work (stream fork, status clear / copy, completion) is paid once per batch.

        out: [B,H,W,3] (allocated when omitted).  tile_rows=(r0,r1) renders only that band of every frame.  With
        `out_bands` — a [B, >= band rows, W, 3] tensor whose frames may be strided views, e.g. the slabs of a sharded
        sweep — only the band is stored, at the top of each slab.  interleave=(stride, phase) with out_bands renders the
        owned tile rows of every frame into compact images (see render()).  want_stats=True also returns every frame's
        statistics (N_v, D, ...); D_f is in them only with stats=True (see render())."""
        scene = self._scene_of(gaussians)
        b = len(cameras)
        if b == 0:
            raise ValueError("no cameras")
        h, w = cameras[0].height, cameras[0].width
        if any(c.height != h or c.width != w for c in cameras):
            raise ValueError("all cameras of a batch must share a resolution")
        r0, r1 = (0, -1) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        cfg = self._c_config(config, (_capi.FLAG_STATS if stats else 0) | (0 if fine_tiles else _capi.FLAG_NO_FINE_TILES))     # (D_f is counted on request only: stats=True)
        if out_bands is not None:
            if out is not None:
                raise ValueError("give out or out_bands, not both")
            stride, phase = (1, 0) if interleave is None else (int(interleave[0]), int(interleave[1]))
            if stride > 1:
                if not 0 <= phase < stride:
                    raise ValueError(f"interleave phase {phase} outside [0, {stride})")
                owned = len(range(phase, cameras[0].tile_rows, stride))
                need, y0 = 16 * (owned if r1 < 0 else min(r1, owned)), 0
                cfg.tile_row_stride, cfg.tile_row_phase = stride, phase
            else:
                if tile_rows is None:
                    raise ValueError("out_bands needs tile_rows (or interleave)")
                if r1 < 0 or r1 > cameras[0].tile_rows:
                    r1 = cameras[0].tile_rows
                if not 0 <= r0 <= r1:
                    raise ValueError(f"tile_rows {tile_rows} is not a band of the frame's {cameras[0].tile_rows} tile rows")
                y0 = r0 * 16
                need = min(r1 * 16, h) - y0
            t = out_bands
            if (t.device != self.device or t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] < b or t.shape[1] < need
                    or tuple(t.shape[2:]) != (w, 3) or t.stride(3) != 1 or t.stride(2) != 3 or t.stride(1) != 3 * w):
                raise ValueError("out_bands must be float32 [>= B, >= band rows, W, 3] on the device with contiguous frames")
            ptr, frame_stride, ret = t.data_ptr() - y0 * w * 3 * 4, int(t.stride(0)), t
        else:
            if interleave is not None:
                raise ValueError("interleave renders into out_bands only")
            if out is None:
                out = torch.zeros((b, h, w, 3), dtype=torch.float32, device=self.device)
            elif (out.device != self.device or out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] < b
                  or tuple(out.shape[1:]) != (h, w, 3) or not out[0].is_contiguous()):
                raise ValueError("out must be float32 [>= B, H, W, 3] on the renderer's device")
            ptr, frame_stride, ret = out.data_ptr(), int(out.stride(0)), out
        arr = self._c_cameras(cameras, scene)
        stats = (_capi.SgsStats * b)() if want_stats else None
        self._lib.check(self._lib.sgs_render_batch_strided(self._ctx, scene.handle, arr.ctypes.data_as(C.POINTER(_capi.SgsCamera)),
                                                           b, C.byref(cfg), r0, r1, ptr, frame_stride, stats, self._stream()), self._ctx)
        if want_stats:
            return ret, [s.as_dict() for s in stats]
        return ret

    def pack_rgba8(self, rgb: torch.Tensor, tonemap: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 [H,W,3] -> uint8 [H,W,4] (alpha 255): the array shape cam.get_rgba() returns.  `out`: a contiguous uint8
        [H,W,4] tensor on the device to write into (e.g. a band of a frame buffer).

        tonemap="reinhard" applies x / (1 + x) first — the operator the reference's stage selects
        (Data/template.usda:102,196).  An optional host-side op, off by default and outside the
        parity contract: the simulator's exposure/white-point settings are not reproduced, frames stay linear otherwise."""
        if tonemap is not None:
            if tonemap != "reinhard":
                raise ValueError("tonemap must be None or 'reinhard'")
            rgb = rgb / (1.0 + rgb.clamp_min(0.0))
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.uint8, device=self.device)
        elif (out.device != self.device or out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (h, w, 4)):
            raise ValueError("out must be a contiguous uint8 [H,W,4] tensor on the renderer's device")
        self._lib.check(self._lib.sgs_pack_rgba8(self._ctx, rgb.contiguous().data_ptr(), out.data_ptr(), w, h,
                                                 self._stream()), self._ctx)
        return out

    # -- host frames (the boundary the reference really has: uint8 arrays on the host) -----------------------------------------
    def host_frames(self, shape, depth: int = 2) -> "HostFrames":
        """A ring of `depth` PINNED uint8 host buffers of `shape` (+ their device-side uint8 twins, a copy stream and events):
        what get_rgba()-shaped callers read frames from.  Cached per (shape, depth)."""
        key = (tuple(int(v) for v in shape), int(depth))
        ring = self._host_rings.get(key) if hasattr(self, "_host_rings") else None
        if ring is None:
            if not hasattr(self, "_host_rings"):
                self._host_rings = {}
            ring = self._host_rings[key] = HostFrames(self, key[0], key[1])
        return ring

    def render_rgba8_host(self, camera: Camera, gaussians, *, config: Optional[RenderConfig] = None, tonemap: Optional[str] = None,
                          output_size=None, resample: str = "bicubic") -> np.ndarray:
        """One frame as the reference's callers receive it: uint8 [H,W,4] (alpha 255) in HOST memory (simple_env.py:1380-1386;
        generate_images.py:428-431).  Render and pack are enqueued back to back on the current stream — the pack kernel writes the
        pinned host buffer itself (no device twin, no copy engine, no pageable staging copy) — and the call waits once.  The array is renderer-owned
        and stays valid until the next-but-one call at this resolution (the reference's callers copy what they keep).
        output_size=(w, h): the frame is rendered at the camera's resolution, resized on the device (resize: `resample`) and packed into
        the pinned ring of the output size — render, resize and pack back to back, still one wait."""
        scene = self._scene_of(gaussians)
        if output_size is not None:
            return self._render_resized_rgba8_host(camera, scene, config, tonemap, (int(output_size[0]), int(output_size[1])), resample)
        ring = self.host_frames((camera.height, camera.width, 4))
        rgb = self.render(camera, scene, config=config, out=ring.rgb_scratch(), sync=False)
        h = ring.submit(rgb, tonemap=tonemap, direct=True)
        try:
            self.sync()                  # the frame's status — and, stream-ordered behind it, pack + copy
        except _capi.SgsError as e:
            if e.code != -4:             # SGS_ERR_OVERFLOW: an asynchronous frame cannot grow the queues; a synchronous one does
                raise
            h.wait()
            rgb = self.render(camera, scene, config=config, out=ring.rgb_scratch(), sync=True)
            h = ring.submit(rgb, tonemap=tonemap, direct=True)
        return h.wait()

    def _render_resized_rgba8_host(self, camera: Camera, scene, config, tonemap, size, resample) -> np.ndarray:
        """render_rgba8_host with output_size: the full-resolution frame goes into a scratch of its own (cached per resolution), the
        resized one into the output ring's."""
        if tonemap is not None and tonemap != "reinhard":
            raise ValueError("tonemap must be None or 'reinhard'")
        ring = self.host_frames((size[1], size[0], 4))
        full = self.__dict__.setdefault("_resize_sources", {})
        key = (camera.height, camera.width)
        if key not in full:
            full[key] = torch.zeros(key + (3,), dtype=torch.float32, device=self.device)

        def issue(sync):
            rgb = self.render(camera, scene, config=config, out=full[key], sync=sync)
            if tonemap is not None:                      # (before the levels are made, as in pack_rgba8)
                rgb = rgb / (1.0 + rgb.clamp_min(0.0))
            return ring.submit(self.resize(rgb, size, filter=resample, out=ring.rgb_scratch()), direct=True)

        h = issue(False)
        try:
            self.sync()
        except _capi.SgsError as e:
            if e.code != -4:             # SGS_ERR_OVERFLOW: see render_rgba8_host
                raise
            h.wait()
            h = issue(True)
        return h.wait()

    # -- JPEG files made on the device (include/sage_gs.h sgs_encode_jpeg) ------------------------------------------------------
    def _encode_jpeg_into(self, rgb: torch.Tensor, n: int, params, out: torch.Tensor, meta: torch.Tensor):
        """sgs_encode_jpeg of the first n frames of rgb [B,H,W,3] on the current stream: files into `out` (uint8, device), offsets and
        sizes into the pinned int64 [2, >= n] `meta`.  Does not synchronise."""
        h, w = int(rgb.shape[1]), int(rgb.shape[2])
        self._lib.check(self._lib.sgs_encode_jpeg(self._ctx, rgb.data_ptr(), w, h, int(n), _frame_stride(rgb, h * w * 3),
                                                  C.byref(params), out.data_ptr(), int(out.numel()), meta[0].data_ptr(), meta[1].data_ptr(),
                                                  self._stream()), self._ctx)

    def _encode_files(self, n: int, cap: int, issue) -> list:
        """The files (bytes, one per frame) of one synchronous encode of n >= 1 frames.  issue(out, meta) enqueues the C call on the
        current stream: files into `out` (uint8 [cap], device), offsets and sizes into the pinned int64 [2, n] `meta`.  Files that do
        not fit `cap` are encoded once more, with the capacity their sizes ask for."""
        meta = torch.zeros((2, n), dtype=torch.int64, pin_memory=True)
        while True:
            out = torch.empty((cap,), dtype=torch.uint8, device=self.device)
            issue(out, meta)
            torch.cuda.current_stream(self.device).synchronize()
            total = int(meta[0, n - 1]) + int(meta[1, n - 1])
            if total <= cap:
                break
            cap = total                                                       # did not fit: the sizes say what does (SGS_ERR_OVERFLOW's figure)
        host = out[:total].cpu().numpy()
        return [host[int(o):int(o) + int(z)].tobytes() for o, z in zip(meta[0].tolist(), meta[1].tolist())]

    def encode_jpeg(self, rgb: torch.Tensor, quality: int = 95, subsampling: str = "4:2:0") -> list:
        """Baseline JPEG files (bytes, one per frame) of float32 [H,W,3] or [B,H,W,3] frames on the device, encoded there: what
        Image.fromarray(get_rgba()[:, :, :3]).save(f, quality=quality) writes for the same picture, same tables, same default
        subsampling (generate_images.py:431-432; vlm_client_modular.py:346-351).  Synchronous: the simple form; jpeg_frames() is the
        pipelined one.  A frame's bytes do not depend on the batch it is encoded in."""
        rgb, _ = _frames_arg(rgb, self.device, torch.float32, (None, None, 3), "rgb")
        n = int(rgb.shape[0])
        if n == 0:
            return []
        params = _capi.jpeg_params(quality, subsampling)
        cap = n * max(1 << 16, int(rgb.shape[1]) * int(rgb.shape[2]))         # a byte a pixel: several times a photographic frame at q95
        return self._encode_files(n, cap, lambda out, meta: self._encode_jpeg_into(rgb, n, params, out, meta))

    def jpeg_frames(self, shape, quality: int = 95, subsampling: str = "4:2:0", depth: int = 3) -> "JpegFrames":
        """A ring of `depth` pinned byte buffers (+ device twins, a copy stream, events) for chunks of up to shape[0] frames of
        shape[1] x shape[2] pixels — JPEG's counterpart of host_frames().  Cached per argument set."""
        key = (tuple(int(v) for v in shape[:3]), int(quality), str(subsampling), int(depth))
        rings = self.__dict__.setdefault("_jpeg_rings", {})
        if key not in rings:
            rings[key] = JpegFrames(self, key[0], key[1], key[2], key[3])
        return rings[key]

    # -- PNG files made on the device (include/sage_gs.h sgs_encode_png) --------------------------------------------------------
    def encode_png(self, frames: torch.Tensor, format: str = "rgb8", depth_scale: float = 10000.0, depth_max: float = 6.5) -> list:
        """PNG files (bytes, one per frame) of float32 frames on the device, encoded there.  format="rgb8": [H,W,3] or [n,H,W,3]
        colour, the picture get_rgba() shows — what the episode's frame_%05d.png sequence holds (simple_env.py:2757-2759).
        format="depth16": [H,W] or [n,H,W] metres as 16-bit grey, np.clip(d, 0, depth_max) * depth_scale -> uint16 — the depth.png
        of the VLM client (vlm_client_modular.py:354-365).  Lossless; synchronous; a frame's bytes do not depend on the batch it is
        encoded in."""
        params = _capi.png_params(format, depth_scale, depth_max)
        rgb = params.format == _capi.PNG_RGB8
        frames, _ = _frames_arg(frames, self.device, torch.float32, (None, None, 3) if rgb else (None, None), "frames")
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if n == 0:
            return []
        frame_floats = h * w * (3 if rgb else 1)
        cap = n * max(1 << 12, frame_floats // 2)                             # half a byte a sample to begin with; the sizes say what fits

        def issue(out, meta):
            self._lib.check(self._lib.sgs_encode_png(self._ctx, frames.data_ptr(), w, h, n, _frame_stride(frames, frame_floats),
                                                     C.byref(params), out.data_ptr(), int(out.numel()), meta[0].data_ptr(), meta[1].data_ptr(),
                                                     self._stream()), self._ctx)
        return self._encode_files(n, cap, issue)

    # -- frames resized on the device (include/sage_gs.h sgs_resize) ------------------------------------------------------------
    def resize(self, frames: torch.Tensor, size, *, filter: str = "bicubic", kind: str = "rgb", clip=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 frames on the device resized there to size = (width, height), as Pillow and Isaac give sizes: what the benchmark's
        low-res mode does on the host (run_benchmark.py:1409-1419, 1441-1451).  kind="rgb": [H,W,3] or [n,H,W,3] colour; the 8-bit
        LEVELS get_rgba() shows are resampled, and the result is a frame on k / 255 that pack_rgba8, encode_jpeg and encode_png show as
        exactly those levels.  kind="depth": [H,W] or [n,H,W]; clip=(lo, hi) is applied to every sample as it is loaded (the reference
        clips in get_depth, then resizes).  filter="bicubic" is PIL's Image.resize(size) at its default resample, bit for bit;
        "linear" is bilinear at half-pixel centres (the sampling cv2 documents for INTER_LINEAR; not pinned to cv2's bytes).
        out: a contiguous float32 tensor of the result's shape on the device to write into.  Asynchronous on the current stream."""
        if kind not in ("rgb", "depth"):
            raise ValueError("kind must be 'rgb' or 'depth'")
        tail = 1 if kind == "rgb" else 0
        if clip is not None and kind != "depth":
            raise ValueError("clip applies to kind='depth' only")
        lo, hi = (float("-inf"), float("inf")) if clip is None else (float(clip[0]), float(clip[1]))
        w, h = int(size[0]), int(size[1])
        params = _capi.resize_params("rgb8" if tail else "f32", filter, w, h, lo, hi)
        frames, single = _frames_arg(frames, self.device, torch.float32, (None, None, 3) if tail else (None, None), "frames")
        n, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        shape = (n, h, w, 3) if tail else (n, h, w)
        res = _out_arg(out, self.device, shape[1:] if single else shape, torch.float32, "out")
        ch = 3 if tail else 1
        self._lib.check(self._lib.sgs_resize(self._ctx, frames.data_ptr(), W, H, n, _frame_stride(frames, H * W * ch),
                                             C.byref(params), res.data_ptr(), h * w * ch, self._stream()), self._ctx)
        return res

    # -- test hooks -------------------------------------------------------------------------------
    def debug_buffer(self, what, dtype):
        have = self._lib.sgs_debug_read(self._ctx, what, None, 0)
        if have < 0:
            self._lib.check(int(have), self._ctx)
        buf = np.zeros(int(have) // np.dtype(dtype).itemsize, dtype)
        if have:
            self._lib.sgs_debug_read(self._ctx, what, buf.ctypes.data, have)
        return buf

    def intermediates(self):
        """(tile_offsets, per-tile sorted Gaussian ids, Gaussian id of each slot, splat words [N_v,12])."""
        off = self.debug_buffer(_capi.BUF_TILE_OFFSETS, np.uint32).astype(np.int64)
        slots = self.debug_buffer(_capi.BUF_SORTED_SLOTS, np.uint32)
        ids = self.debug_buffer(_capi.BUF_SLOT_IDS, np.uint32)
        splats = self.debug_buffer(_capi.BUF_SPLATS, np.uint32).reshape(-1, 12)
        live = ids != 0xFFFFFFFF
        return off, ids[slots].astype(np.int64), ids[live].astype(np.int64), splats[live]

    # -- collision-mesh depth (include/sage_gs.h sgs_render_mesh_depth*) ---------------------------------------------------------
    def upload_mesh(self, vertices, triangles, model_to_world=None, labels=None) -> Mesh:
        """vertices [V,3] and triangles [F,3] (int) — NumPy arrays or tensors, on the host or on a device.  The non-rigid part of
        model_to_world (a scale, a shear: USD xformOp:scale / metersPerUnit) is baked into the vertices here, so that the view the
        library gets stays rigid; the rotation + translation travel with the Mesh and are applied by moving the camera.
        labels: int32 [F], one object label >= 0 per triangle for render_mesh_ids (set_mesh_labels); None: the triangle's index."""
        rigid, bake = (None, None) if model_to_world is None else _split_model_to_world(model_to_world)
        v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
        t = triangles.detach().cpu().numpy() if isinstance(triangles, torch.Tensor) else np.asarray(triangles)
        v = np.asarray(v, np.float64).reshape(-1, 3)
        if t.size and (not np.issubdtype(t.dtype, np.integer)):
            raise ValueError("triangles must be integer indices")
        t = np.ascontiguousarray(np.asarray(t, np.int64).reshape(-1, 3))
        if t.size and (t.min() < -(1 << 31) or t.max() >= (1 << 31)):
            raise ValueError("triangle indices do not fit int32")
        if bake is not None:
            v = v @ bake.T
        vf = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(self.device)
        tf = torch.from_numpy(t.astype(np.int32)).to(self.device)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            h = C.c_void_p()
            self._lib.check(self._lib.sgs_mesh_upload(self._ctx, int(vf.shape[0]), vf.data_ptr() if vf.numel() else None, int(tf.shape[0]),
                                                      tf.data_ptr() if tf.numel() else None, 1, C.byref(h)), self._ctx)
        mesh = Mesh(self, h, int(vf.shape[0]), int(tf.shape[0]), rigid)
        if labels is not None:
            try:
                self.set_mesh_labels(mesh, labels)
            except Exception:
                mesh.free()
                raise
        return mesh

    def _mesh_of(self, mesh: Mesh) -> Mesh:
        if not isinstance(mesh, Mesh) or mesh._r is not self:
            raise ValueError("the mesh must be a Mesh uploaded by this Renderer (upload_mesh)")
        if mesh.handle is None:
            raise ValueError("this Mesh has been freed")
        return mesh

    def render_mesh_depth(self, camera: Camera, mesh: Mesh, *, config: Optional[RenderConfig] = None, tile_rows=None,
                          out: Optional[torch.Tensor] = None, timing=False) -> torch.Tensor:
        """float32 [H,W] on the device: per pixel the camera-space z (distance to the image plane) of the nearest triangle of `mesh`
        hit with near < z <= far (config; both faces count), +inf where none is.  tile_rows=(r0,r1): only that band of 16-pixel tile
        rows is written (the rest of `out` is left as it was).  Statistics in last_stats."""
        mesh = self._mesh_of(mesh)
        h, w = camera.height, camera.width
        out = _out_arg(out, self.device, (h, w), torch.float32, "out", zero=True)           # zeros: a band leaves the other rows alone
        r0, r1 = (0, -1) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        cfg = self._c_config(config, _capi.FLAG_TIMING if timing else 0)
        cam = self._c_camera(camera, mesh)
        st = _capi.SgsStats()
        self._lib.check(self._lib.sgs_render_mesh_depth(self._ctx, mesh.handle, C.byref(cam), C.byref(cfg), r0, r1, out.data_ptr(),
                                                        C.byref(st), self._stream()), self._ctx)
        self.last_stats = st.as_dict()
        return out

    def render_mesh_depth_batch(self, cameras: Sequence[Camera], mesh: Mesh, *, config: Optional[RenderConfig] = None,
                                out: Optional[torch.Tensor] = None, timing=False, want_stats=False):
        """render_mesh_depth for B cameras of one resolution in one call: float32 [B,H,W] (and the frames' statistics with want_stats).
        Every frame equals the one render_mesh_depth draws, bit for bit."""
        mesh = self._mesh_of(mesh)
        b = len(cameras)
        if b == 0:
            raise ValueError("no cameras")
        h, w = cameras[0].height, cameras[0].width
        if any(c.height != h or c.width != w for c in cameras):
            raise ValueError("all cameras of a batch must share a resolution")
        out = _out_arg(out, self.device, (b, h, w), torch.float32, "out", zero=True)
        cfg = self._c_config(config, _capi.FLAG_TIMING if timing else 0)
        arr = self._c_cameras(cameras, mesh)
        stats = (_capi.SgsStats * b)()
        self._lib.check(self._lib.sgs_render_mesh_depth_batch(self._ctx, mesh.handle, arr.ctypes.data, b, C.byref(cfg), out.data_ptr(),
                                                              stats, self._stream()), self._ctx)
        self.last_stats = stats[b - 1].as_dict()
        return (out, [s.as_dict() for s in stats]) if want_stats else out

    # -- collision-mesh object ids (include/sage_gs.h sgs_render_mesh_ids*: this project's own channel, the reference has none) ----
    def set_mesh_labels(self, mesh: Mesh, labels):
        """One int32 label per triangle of `mesh`, 0 <= label <= 2^31 - 2 (typically mesh.read_usda_mesh(return_prims=True)'s tri_prim) —
        a NumPy array or a tensor, on the host or on the device; copied.  None restores the default: a triangle's label is its index.
        A wrong length, a dtype other than int32 and (for host arrays) labels out of range are refused here; for a device tensor the
        range is checked by the library on the device.  A refused call leaves the mesh's labels as they were."""
        mesh = self._mesh_of(mesh)
        if labels is None:
            self._lib.check(self._lib.sgs_mesh_set_labels(self._ctx, mesh.handle, None, 0), self._ctx)
            return
        if isinstance(labels, torch.Tensor):
            if labels.dtype != torch.int32:
                raise ValueError(f"labels must be int32 (got {labels.dtype})")
            lab = labels.detach().reshape(-1)
        else:
            a = np.asarray(labels)
            if a.dtype != np.int32:
                raise ValueError(f"labels must be int32 (got {a.dtype})")
            if a.size and (int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 2):
                raise ValueError("labels must lie in [0, 2^31 - 2]")
            lab = torch.from_numpy(np.ascontiguousarray(a.reshape(-1)))
        if lab.numel() != mesh.n_triangles:
            raise ValueError(f"{lab.numel()} labels for a mesh of {mesh.n_triangles} triangles")
        lab = lab.to(self.device).contiguous()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            self._lib.check(self._lib.sgs_mesh_set_labels(self._ctx, mesh.handle, lab.data_ptr() if lab.numel() else None, 1), self._ctx)

    def render_mesh_ids(self, camera: Camera, mesh: Mesh, *, config: Optional[RenderConfig] = None, tile_rows=None,
                        out: Optional[torch.Tensor] = None, out_depth: Optional[torch.Tensor] = None, return_depth=False, stats=False,
                        timing=False):
        """int32 [H,W] on the device: per pixel the label of the triangle of `mesh` whose hit render_mesh_depth reports — the nearest
        hit with near < z <= far, the least label among hits at bit-equal z — and -1 (_capi.ID_NONE) where nothing is hit.
        return_depth=True: (ids, depth), depth bit for bit render_mesh_depth's frame.  tile_rows, out (ids) and out_depth as
        render_mesh_depth's: a band leaves the other rows of both alone.  stats=True appends the frame's statistics (also in
        last_stats).  The channel is this project's own definition (the reference has no such observation)."""
        mesh = self._mesh_of(mesh)
        h, w = camera.height, camera.width
        out = _out_arg(out, self.device, (h, w), torch.int32, "out", zero=True)
        depth = _out_arg(out_depth, self.device, (h, w), torch.float32, "out_depth", zero=True) if (return_depth or out_depth is not None) else None
        r0, r1 = (0, -1) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        cfg = self._c_config(config, _capi.FLAG_TIMING if timing else 0)
        cam = self._c_camera(camera, mesh)
        st = _capi.SgsStats()
        self._lib.check(self._lib.sgs_render_mesh_ids(self._ctx, mesh.handle, C.byref(cam), C.byref(cfg), r0, r1,
                                                      depth.data_ptr() if depth is not None else None, out.data_ptr(), C.byref(st),
                                                      self._stream()), self._ctx)
        self.last_stats = st.as_dict()
        ret = (out, depth) if return_depth else (out,)
        if stats:
            ret += (self.last_stats,)
        return ret if len(ret) > 1 else ret[0]

    def render_mesh_ids_batch(self, cameras: Sequence[Camera], mesh: Mesh, *, config: Optional[RenderConfig] = None,
                              out: Optional[torch.Tensor] = None, out_depth: Optional[torch.Tensor] = None, return_depth=False,
                              timing=False, want_stats=False):
        """render_mesh_ids for B cameras of one resolution in one call: int32 [B,H,W], or (ids, depth [B,H,W]) with return_depth, and
        the frames' statistics last with want_stats.  Every frame equals the one render_mesh_ids draws, bit for bit."""
        mesh = self._mesh_of(mesh)
        b = len(cameras)
        if b == 0:
            raise ValueError("no cameras")
        h, w = cameras[0].height, cameras[0].width
        if any(c.height != h or c.width != w for c in cameras):
            raise ValueError("all cameras of a batch must share a resolution")
        out = _out_arg(out, self.device, (b, h, w), torch.int32, "out", zero=True)
        depth = _out_arg(out_depth, self.device, (b, h, w), torch.float32, "out_depth", zero=True) if (return_depth or out_depth is not None) else None
        cfg = self._c_config(config, _capi.FLAG_TIMING if timing else 0)
        arr = self._c_cameras(cameras, mesh)
        st = (_capi.SgsStats * b)()
        self._lib.check(self._lib.sgs_render_mesh_ids_batch(self._ctx, mesh.handle, arr.ctypes.data, b, C.byref(cfg),
                                                            depth.data_ptr() if depth is not None else None, out.data_ptr(), st,
                                                            self._stream()), self._ctx)
        self.last_stats = st[b - 1].as_dict()
        ret = (out, depth) if return_depth else (out,)
        if want_stats:
            ret += ([s.as_dict() for s in st],)
        return ret if len(ret) > 1 else ret[0]

    # -- the visible-object table of id frames (include/sage_gs.h sgs_object_table: this project's own definition, as the ids are) ----
    def _id_frames_of(self, ids: torch.Tensor, depth: Optional[torch.Tensor]):
        ids, single = _frames_arg(ids, self.device, torch.int32, (None, None), "ids", min_frames=1)
        if single and depth is not None and depth.dim() == 2:
            depth = depth.unsqueeze(0)
        if depth is not None and (depth.device != self.device or depth.dtype != torch.float32 or tuple(depth.shape) != tuple(ids.shape)
                                  or depth.stride() != ids.stride()):
            raise ValueError("depth must be float32 of the ids' shape and strides on the renderer's device")
        return ids, depth

    def object_table(self, ids: torch.Tensor, depth: Optional[torch.Tensor] = None, *, n_labels: int, out=None):
        """The visible-object table of int32 id frames [H,W] or [B,H,W] on the device (render_mesh_ids*'s, or any other), reduced there
        in one launch for the whole batch: (rows, counts).  rows is int32 [B, n_labels, 10] whose bytes are sgs_object_row
        (_capi.OBJECT_ROW_DTYPE): row k of a frame describes label k — pixels, tight box (x_min, y_min, x_end, y_end: ends exclusive),
        the least depth of `depth` (float32, the ids' shape; +inf without it) and the sums of x and y; counts is int32 [B, 2]: the
        pixels equal to -1 (nothing hit) and the pixels whose id is neither -1 nor a label below n_labels, which enter no row.
        out=(rows, counts): contiguous tensors of those shapes to write into.  Nothing is copied to the host; asynchronous on the
        current stream.  A frame's table does not depend on the batch it is in.  This project's own definition: the reference has no
        such observation."""
        ids, depth = self._id_frames_of(ids, depth)
        b, h, w = int(ids.shape[0]), int(ids.shape[1]), int(ids.shape[2])
        n_labels = int(n_labels)
        if n_labels < 1:
            raise ValueError("n_labels must be at least 1")
        rows, counts = (None, None) if out is None else out
        rows = _out_arg(rows, self.device, (b, n_labels, _capi.OBJECT_ROW_WORDS), torch.int32, "out[0]")
        counts = _out_arg(counts, self.device, (b, 2), torch.int32, "out[1]")
        self._lib.check(self._lib.sgs_object_table(self._ctx, ids.data_ptr(), depth.data_ptr() if depth is not None else None, b, h, w,
                                                   _frame_stride(ids, h * w), n_labels, rows.data_ptr(), counts.data_ptr(),
                                                   self._stream()), self._ctx)
        return rows, counts

    def visible_objects(self, ids: torch.Tensor, depth: Optional[torch.Tensor] = None, *, n_labels: int, min_pixels: int = 1) -> list:
        """Per frame a NumPy structured array (_capi.VISIBLE_OBJECT_DTYPE: `label` and sgs_object_row's fields) of the labels that cover
        at least min_pixels pixels, by ascending label: object_table on the device, the rows selected there, and only those copied to
        the host.  ValueError (naming the frame and the count) when a frame holds ids that are neither -1 nor below n_labels."""
        rows, counts = self.object_table(ids, depth, n_labels=n_labels)
        where = torch.nonzero(rows[:, :, 0] >= max(int(min_pixels), 1))           # [K, 2]: (frame, label), in that order
        picked = rows[where[:, 0], where[:, 1]]
        counts_h, where_h, picked_h = counts.cpu().numpy(), where.cpu().numpy(), picked.cpu().numpy()
        bad = np.flatnonzero(counts_h[:, 1])
        if len(bad):
            raise ValueError(f"frame {int(bad[0])}: {int(counts_h[bad[0], 1].view(np.uint32))} pixels hold ids that are neither -1 nor below n_labels = {int(n_labels)}")
        out = np.zeros(len(where_h), _capi.VISIBLE_OBJECT_DTYPE)
        out["label"] = where_h[:, 1]
        rec = np.ascontiguousarray(picked_h).view(_capi.OBJECT_ROW_DTYPE).reshape(-1)
        for name in _capi.OBJECT_ROW_DTYPE.names:
            out[name] = rec[name]
        cuts = np.searchsorted(where_h[:, 0], np.arange(rows.shape[0] + 1))
        return [out[cuts[f]:cuts[f + 1]] for f in range(rows.shape[0])]

    # -- image similarity of frames against a target picture (include/sage_gs.h sgs_image_similarity: this project's own definition) --
    def _target_levels(self, target) -> torch.Tensor:
        """`target` as uint8 [H,W,3] or [B,H,W,3] on the device: a tensor there already, or a NumPy array or PIL image, uploaded."""
        if not isinstance(target, torch.Tensor):
            if hasattr(target, "convert") and hasattr(target, "size"):                # a PIL image
                target = np.asarray(target.convert("RGB"))
            target = np.asarray(target)
            if target.dtype != np.uint8:
                raise ValueError(f"target must hold uint8 levels, not {target.dtype}")
            target = torch.from_numpy(np.array(target, order="C")).to(self.device)                  # (a copy: PIL's arrays are read-only)
        if target.dtype != torch.uint8:
            raise ValueError(f"target must hold uint8 levels, not {target.dtype}")
        if target.device != self.device or target.dim() not in (3, 4) or target.shape[-1] != 3 or not target[(0,) * (target.dim() - 3)].is_contiguous():
            raise ValueError("target must be uint8 [H,W,3] or [B,H,W,3] on the renderer's device with contiguous pictures")
        return target

    def image_similarity(self, frames: torch.Tensor, target) -> np.ndarray:
        """Windowed SSIM and squared error of float32 frames [H,W,3] or [B,H,W,3] on the device against `target`: uint8 levels
        [H,W,3] (one picture for every frame) or [B,H,W,3] (frame f against picture f) as a tensor on the device, or a NumPy array
        or PIL image, which is uploaded.  One launch for the whole batch; 64 bytes per frame come back.  Returns a NumPy structured
        array with one record per frame (_capi.SIMILARITY_DTYPE): sgs_similarity_row's fields — ssim_q[3], sse[3], n_windows,
        n_pixels, exact integers — and the host divisions ssim (the mean over the three channels, 1.0 for identical pictures),
        ssim_rgb[3], mse (in levels squared) and psnr (dB, inf at zero error).  The frame's levels are the ones get_rgba() shows.
        ValueError on a size or dtype mismatch: nothing is ever resized here.  This project's own definition: the reference names
        the measure for ImgNav (task_types.py:183-208) and returns a placeholder."""
        frames, _ = _frames_arg(frames, self.device, torch.float32, (None, None, 3), "frames", min_frames=1)
        b, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        target = self._target_levels(target)
        if tuple(target.shape[-3:]) != (h, w, 3):
            raise ValueError(f"target is {int(target.shape[-2])} x {int(target.shape[-3])}, the frames are {w} x {h}: resize one of them first")
        if target.dim() == 4 and int(target.shape[0]) != b:
            raise ValueError(f"{int(target.shape[0])} targets for {b} frames")
        if w < _capi.SIMILARITY_WINDOW or h < _capi.SIMILARITY_WINDOW:
            raise ValueError(f"frames of {w} x {h} hold no {_capi.SIMILARITY_WINDOW} x {_capi.SIMILARITY_WINDOW} window")
        size = 3 * h * w
        t_stride = 0 if target.dim() == 3 else _frame_stride(target, size)
        rows = torch.empty((b, 8), dtype=torch.int64, device=self.device)
        self._lib.check(self._lib.sgs_image_similarity(self._ctx, frames.data_ptr(), w, h, b, _frame_stride(frames, size),
                                                       target.data_ptr(), t_stride, rows.data_ptr(), self._stream()), self._ctx)
        raw = np.ascontiguousarray(rows.cpu().numpy()).view(_capi.SIMILARITY_ROW_DTYPE).reshape(b)
        out = np.zeros(b, _capi.SIMILARITY_DTYPE)
        for name in _capi.SIMILARITY_ROW_DTYPE.names:
            out[name] = raw[name]
        one = float(1 << _capi.SIMILARITY_Q_BITS)
        n_win, n_pix = raw["n_windows"].astype(np.float64), raw["n_pixels"].astype(np.float64)
        out["ssim_rgb"] = raw["ssim_q"].astype(np.float64) / (n_win[:, None] * one)
        out["ssim"] = np.array([float(int(q.sum())) for q in raw["ssim_q"]]) / (3.0 * n_win * one)
        out["mse"] = np.array([float(int(e.sum())) for e in raw["sse"]]) / (3.0 * n_pix)
        with np.errstate(divide="ignore"):
            out["psnr"] = np.where(out["mse"] > 0, 10.0 * np.log10(255.0 * 255.0 / np.where(out["mse"] > 0, out["mse"], 1.0)), np.inf)
        return out

    # -- the top-down seen map of depth frames (include/sage_gs.h sgs_topdown_map: this project's own definition) ------------------
    def pix_to_map(self, cameras, model_to_map=None) -> torch.Tensor:
        """float32 [B,12] on the device: per camera the twelve numbers sgs_topdown_map unprojects a depth frame with — the rows of
        map_from_cam . [(1/fx, 0, (0.5 - cx)/fx); (0, 1/fy, (0.5 - cy)/fy); (0, 0, 1)] (the mesh path's ray through the pixel
        centre), then the camera's position in the map.  Computed in NumPy fp64 from each camera's intrinsics and the inverse of its
        rigid view, then rounded once.  model_to_map: a 3x4 (or 4x4) taking the space the view maps FROM — the world of the
        cameras' poses — to the map, whose third coordinate is the height; default the identity.  `cameras`: a Camera or a sequence."""
        cams = [cameras] if isinstance(cameras, Camera) else list(cameras)
        if not cams:
            raise ValueError("no cameras")
        m = np.eye(4)
        if model_to_map is not None:
            mm = np.asarray(model_to_map, np.float64)
            if mm.shape not in ((3, 4), (4, 4)) or not np.isfinite(mm).all():
                raise ValueError("model_to_map must be a finite 3x4 (or 4x4) matrix")
            m[:3] = mm[:3]
        out = np.empty((len(cams), 12), np.float64)
        for k, c in enumerate(cams):
            view = np.asarray(c.view.detach().cpu().numpy() if isinstance(c.view, torch.Tensor) else c.view, np.float64).reshape(4, 4)
            c2m = m @ np.linalg.inv(_rigid(view))
            fx, fy, cx, cy = float(c.fx), float(c.fy), float(c.cx), float(c.cy)
            K = np.array([[1.0 / fx, 0.0, (0.5 - cx) / fx], [0.0, 1.0 / fy, (0.5 - cy) / fy], [0.0, 0.0, 1.0]])
            out[k, :9] = (c2m[:3, :3] @ K).reshape(9)
            out[k, 9:] = c2m[:3, 3]
        return torch.from_numpy(out.astype(np.float32)).to(self.device)

    def topdown_map(self, depth: torch.Tensor, cameras_or_P, grid: Optional[TopdownGrid] = None, out=None, clear: bool = True):
        """The top-down seen map of float32 depth frames [H,W] or [B,H,W] on the device (render_mesh_depth*'s, or any other distance to
        the image plane), accumulated there in one launch for the whole batch: (grid, counts).  grid is uint32-valued int32
        [ny, nx, 2] — per cell the free hits and the occupied hits — and counts int32 [B, 4]: per frame the pixels whose depth is
        outside [min_z, max_z], outside the grid, inside it but in neither height band, and binned.  cameras_or_P: the frames'
        cameras (pix_to_map is taken of them, with the identity as model_to_map) or a float32 [B,12] tensor that pix_to_map made.
        grid: a TopdownGrid (default TopdownGrid()).  out=(grid, counts): contiguous int32 tensors of those shapes to write into;
        clear=False adds to what out's grid holds (it needs out=).  Nothing is copied to the host; asynchronous on the current
        stream.  Every count is an integer: the map does not depend on the batch, the order of the frames or how they are split
        over calls.  This project's own definition: the reference counts the cells the agent stood in (measures.py:399-437)."""
        g = TopdownGrid() if grid is None else grid
        depth, _ = _frames_arg(depth, self.device, torch.float32, (None, None), "depth", min_frames=1)
        b, h, w = int(depth.shape[0]), int(depth.shape[1]), int(depth.shape[2])
        if isinstance(cameras_or_P, torch.Tensor):
            P = cameras_or_P
            if P.device != self.device or P.dtype != torch.float32 or tuple(P.shape) != (b, 12) or not P.is_contiguous():
                raise ValueError(f"P must be a contiguous float32 [{b}, 12] tensor on the renderer's device")
        else:
            cams = [cameras_or_P] if isinstance(cameras_or_P, Camera) else list(cameras_or_P)
            if len(cams) != b or any(c.width != w or c.height != h for c in cams):
                raise ValueError(f"{len(cams)} cameras for {b} frames of {w} x {h}")
            P = self.pix_to_map(cams)
        if out is None and not clear:
            raise ValueError("clear=False adds to a grid: pass it as out=(grid, counts)")
        cells, counts = (None, None) if out is None else out
        cells = _out_arg(cells, self.device, (int(g.ny), int(g.nx), 2), torch.int32, "out[0]")
        counts = _out_arg(counts, self.device, (b, 4), torch.int32, "out[1]")
        params = g.c_params(clear)
        self._lib.check(self._lib.sgs_topdown_map(self._ctx, depth.data_ptr(), w, h, b, _frame_stride(depth, h * w),
                                                  P.data_ptr(), C.byref(params), cells.data_ptr(), counts.data_ptr(), self._stream()), self._ctx)
        return cells, counts

    def topdown_summary(self, grid: torch.Tensor, min_hits: int = 1, cell_size: Optional[float] = None) -> dict:
        """What a seen map holds, reduced on the device (32 bytes come back): a dict of Python ints — occupied_cells (occupied hits
        >= min_hits), free_cells (free hits >= min_hits and occupied hits below it), free_hits, occupied_hits — plus
        seen_cells = occupied_cells + free_cells and, given the grid's cell_size, seen_area_m2 = seen_cells cell_size^2."""
        if (not isinstance(grid, torch.Tensor) or grid.device != self.device or grid.dtype != torch.int32 or grid.dim() != 3 or grid.shape[2] != 2
                or not grid.is_contiguous()):
            raise ValueError("grid must be a contiguous int32 [ny, nx, 2] tensor on the renderer's device")
        if int(min_hits) < 1 or int(min_hits) > 0xFFFFFFFF:
            raise ValueError("min_hits must be within 1 .. 2^32 - 1")
        out = torch.empty(4, dtype=torch.int64, device=self.device)
        self._lib.check(self._lib.sgs_topdown_summary(self._ctx, grid.data_ptr(), int(grid.shape[1]), int(grid.shape[0]), int(min_hits),
                                                      out.data_ptr(), self._stream()), self._ctx)
        occ, free, free_hits, occ_hits = (int(v) for v in out.cpu().numpy().view(np.uint64))
        d = {"occupied_cells": occ, "free_cells": free, "free_hits": free_hits, "occupied_hits": occ_hits, "seen_cells": occ + free}
        d["seen_area_m2"] = None if cell_size is None else (occ + free) * float(cell_size) ** 2
        return d

    # -- the clearance map: where an agent can stand (include/sage_gs.h sgs_clearance_map, sgs_clearance_query) ------------------------
    def clearance_map(self, src: torch.Tensor, *, kind: Optional[str] = None, min_hits: int = 1, unseen_blocks: bool = False,
                      max_d2: int = 0, out=None):
        """The exact squared Euclidean distance transform of obstacle grids on the device, a whole batch in one call: (d2, counts).
        src: a mask — uint8 or bool [ny,nx] or [B,ny,nx], non-zero is an obstacle — or a seen map — int32 [ny,nx,2] or [B,ny,nx,2]
        as topdown_map writes it, a cell an obstacle iff its occupied hits >= min_hits, with unseen_blocks also when neither count
        reaches min_hits.  kind ("mask" / "topdown") is inferred from the dtype and shape.  d2 is uint32-valued int32 of src's map
        shape — cells^2 to the nearest obstacle, 0 on one, -1 (SGS_CLEARANCE_NONE) all over a map without any — and counts int32
        [4] or [B,4]: obstacle cells, cells with 0 < d2 <= max_d2, cells with max_d2 < d2 < NONE, cells equal to NONE.
        out=(d2, counts): contiguous int32 tensors of those shapes.  Nothing is copied to the host; asynchronous on the current
        stream.  All integer: a map's d2 does not depend on the batch it is issued in."""
        if kind is None:
            kind = "topdown" if getattr(src, "dtype", None) == torch.int32 else "mask"
        if kind == "mask":
            maps, batched, b, ny, nx, stride = _maps_arg(src, self.device, torch.uint8, 1, "a mask")
            source = _capi.CLEARANCE_SRC_MASK8
            if unseen_blocks:
                raise ValueError("unseen_blocks has a meaning for a seen map only")
        elif kind == "topdown":
            maps, batched, b, ny, nx, stride = _maps_arg(src, self.device, torch.int32, 2, "a seen map")
            source = _capi.CLEARANCE_SRC_TOPDOWN
        else:
            raise ValueError(f"unknown kind {kind!r}: 'mask' or 'topdown'")
        if not (1 <= int(min_hits) <= 0xFFFFFFFF and 0 <= int(max_d2) <= 0xFFFFFFFF):
            raise ValueError("min_hits must be within 1 .. 2^32 - 1 and max_d2 within 0 .. 2^32 - 1")
        shape, cshape = ((b, ny, nx), (b, 4)) if batched else ((ny, nx), (4,))
        d2 = _out_arg(None if out is None else out[0], self.device, shape, torch.int32, "out[0]")
        counts = _out_arg(None if out is None else out[1], self.device, cshape, torch.int32, "out[1]")
        work = torch.empty((b, ny, nx), dtype=torch.int32, device=self.device)
        params = _capi.SgsClearanceParams(nx, ny, source, _capi.CLEARANCE_UNSEEN_BLOCKS if unseen_blocks else 0,
                                          int(min_hits) if source == _capi.CLEARANCE_SRC_TOPDOWN else 0, int(max_d2), 0)
        self._lib.check(self._lib.sgs_clearance_map(self._ctx, maps.data_ptr(), b, stride,
                                                    C.byref(params), work.data_ptr(), d2.data_ptr(), counts.data_ptr(), self._stream()), self._ctx)
        return d2, counts

    def clearance_query(self, d2: torch.Tensor, frame, segments, n_samples: int = 10) -> torch.Tensor:
        """The reference's position and path checks for n segments in one launch: int64 [n,2] on the device — per segment the index
        of its first colliding sample (from 1) or 0, and the d2 under its end point (SGS_CLEARANCE_NONE = 4294967295 when that is
        outside the map beyond the margin).  d2: one map, int32 [ny,nx] as clearance_map returns it; frame: a
        sage_gs.clearance.ClearanceFrame; segments: float64 [n,4] (x0, y0, x1, y1), a tensor on the device or anything
        np.asarray takes.  n_samples <= 1 checks the end point alone.  A NaN or infinite coordinate collides."""
        if not isinstance(d2, torch.Tensor) or d2.device != self.device or d2.dtype != torch.int32 or d2.dim() != 2 or not d2.is_contiguous():
            raise ValueError("d2 must be a contiguous int32 [ny,nx] tensor on the renderer's device")
        segs = _rows_arg(segments, self.device, torch.float64, 4, "segments")
        n = int(segs.shape[0])
        out = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        f = frame.c_frame(n_samples)
        self._lib.check(self._lib.sgs_clearance_query(self._ctx, d2.data_ptr(), int(d2.shape[1]), int(d2.shape[0]), segs.data_ptr(), n,
                                                      C.byref(f), out.data_ptr(), self._stream()), self._ctx)
        return out.to(torch.int64) & 0xFFFFFFFF

    # -- geodesic fields and shortest paths (include/sage_gs.h sgs_geodesic_field, sgs_geodesic_path) ---------------------------------
    def _geodesic_source(self, src, max_d2):
        dtype = getattr(src, "dtype", None)
        if dtype in (torch.uint8, torch.bool):
            source = _capi.GEODESIC_SRC_MASK8
            if max_d2 is not None:
                raise ValueError("max_d2 has a meaning for a d2 map only")
        elif dtype == torch.int32:
            source = _capi.GEODESIC_SRC_D2
            if max_d2 is None:
                raise ValueError("a d2 map needs max_d2: a cell is blocked iff d2 <= max_d2")
        else:
            raise ValueError("src must be a mask (uint8 or bool) or a d2 map (int32 as clearance_map returns it), [ny,nx] or [B,ny,nx]")
        maps, _, b, ny, nx, stride = _maps_arg(src, self.device, torch.uint8 if source == _capi.GEODESIC_SRC_MASK8 else torch.int32, 1, "src")
        if max(nx, ny) > _capi.GEODESIC_MAX_N:
            raise ValueError(f"src must hold maps of 1 .. {_capi.GEODESIC_MAX_N} cells a side")
        if max_d2 is not None and not 0 <= int(max_d2) <= 0xFFFFFFFF:
            raise ValueError("max_d2 must be within 0 .. 2^32 - 1")
        return maps, source, b, ny, nx, stride

    @staticmethod
    def _geodesic_table(rows, width, what):
        t = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, width) if width > 1 else np.asarray(rows, np.int64).reshape(-1))
        if len(t) < 1 or np.abs(t).max() > 0x7FFFFFFF:
            raise ValueError(f"{what} must hold at least one row of int32 values")
        return np.ascontiguousarray(t.astype(np.int32))

    def geodesic_field(self, src: torch.Tensor, seeds, field_map=None, max_d2: Optional[int] = None, rounds: Optional[int] = None):
        """Geodesic distance fields on the device: for every cell of a blocked grid the pair (a, b) = (straight steps, diagonal steps)
        of the cheapest 8-connected walk to any seed of its field — cost a + b sqrt(2), compared exactly in integers, a diagonal step
        needing only its two end cells free.  src: a mask (uint8 or bool, non-zero is blocked) or a d2 map (int32 as clearance_map
        returns it, blocked iff d2 <= max_d2), [ny,nx] or [B,ny,nx].  seeds: [(field, i, j)] on the host; field_map: the map of every
        field (default: one field per map).  Returns (steps, blocked_seeds): steps int32 [n_fields,ny,nx,2], uint32-valued — -1 in
        both words (SGS_GEODESIC_NONE) where a cell is blocked or unreachable —, and per field the seeds ignored because their cell
        is blocked.  This method owns the loop: a first call of `rounds` rounds (default 2 (tiles_x + tiles_y)), the status read
        back, and SGS_GEODESIC_CONTINUE calls of as many rounds until no tile of any field is dirty.  Raises if that takes more than
        nx * ny rounds, which no map needs.  The result does not depend on `rounds`: the field is the relaxation's unique fixed point."""
        maps, source, b, ny, nx, stride = self._geodesic_source(src, max_d2)
        fm = self._geodesic_table(np.arange(b) if field_map is None else field_map, 1, "field_map")
        sd = self._geodesic_table(seeds, 3, "seeds")
        nf = len(fm)
        T = int(self._lib.sgs_geodesic_tile())
        per_call = 2 * ((nx + T - 1) // T + (ny + T - 1) // T) if rounds is None else int(rounds)
        words = int(self._lib.sgs_geodesic_state_words(nx, ny, nf))
        if words < 0 or per_call < 1:
            raise ValueError(f"{nf} fields of {nx} x {ny} cells, {per_call} rounds a call: outside what sgs_geodesic_field takes")
        dist = torch.empty((nf, ny, nx, 2), dtype=torch.int32, device=self.device)
        state = torch.empty((words,), dtype=torch.int32, device=self.device)
        status = torch.empty((nf, 2), dtype=torch.int32, device=self.device)
        total, flags = 0, 0
        while True:
            params = _capi.SgsGeodesicParams(nx, ny, source, int(max_d2 or 0), flags, 0)
            self._lib.check(self._lib.sgs_geodesic_field(self._ctx, maps.data_ptr(), b, stride, C.byref(params), fm.ctypes.data, nf, sd.ctypes.data,
                                                         len(sd), dist.data_ptr(), state.data_ptr(), per_call, status.data_ptr(), self._stream()), self._ctx)
            total += per_call
            st = status.cpu().numpy().view(np.uint32)
            if not st[:, 0].any():
                break
            if total > nx * ny:
                raise RuntimeError(f"geodesic_field: tiles are still dirty after {total} rounds on a map of {nx} x {ny}")
            flags = _capi.GEODESIC_CONTINUE
        self.last_geodesic_rounds = total
        return dist, st[:, 1].astype(np.int64)

    def geodesic_path(self, src: torch.Tensor, steps: torch.Tensor, queries, field_map=None, max_d2: Optional[int] = None, max_len: Optional[int] = None):
        """Shortest paths down a final field, one thread per query, one launch: (cells, info).  src, field_map, max_d2: as given to
        geodesic_field; steps: what it returned; queries: [(field, i, j)], a tensor on the device or anything np.asarray takes.
        cells int32 [n,max_len,2] = (i, j) from the start to a seed — max_len defaults to nx * ny, so give one —, info int64 [n,2]:
        the cells written and a status (0 ok, 1 the start is blocked or unreachable, 2 truncated at max_len, 3 no such field or
        cell, 4 the field is not final).  Among equal-cost walks the one the fixed neighbour order picks."""
        maps, source, b, ny, nx, stride = self._geodesic_source(src, max_d2)
        fm = self._geodesic_table(np.arange(b) if field_map is None else field_map, 1, "field_map")
        if not isinstance(steps, torch.Tensor) or steps.device != self.device or steps.dtype != torch.int32 or not steps.is_contiguous() or \
                tuple(steps.shape) != (len(fm), ny, nx, 2):
            raise ValueError(f"steps must be a contiguous int32 [{len(fm)},{ny},{nx},2] tensor on the renderer's device")
        q = _rows_arg(queries if isinstance(queries, torch.Tensor) else np.asarray(queries, np.int64).reshape(-1, 3), self.device, torch.int32, 3, "queries")
        n = int(q.shape[0])
        max_len = nx * ny if max_len is None else int(max_len)
        if max_len < 1:
            raise ValueError("max_len must be >= 1")
        cells = torch.full((n, max_len, 2), -1, dtype=torch.int32, device=self.device)
        info = torch.empty((n, 2), dtype=torch.int32, device=self.device)
        params = _capi.SgsGeodesicParams(nx, ny, source, int(max_d2 or 0), 0, 0)
        self._lib.check(self._lib.sgs_geodesic_path(self._ctx, maps.data_ptr(), b, stride, C.byref(params), fm.ctypes.data, len(fm), steps.data_ptr(),
                                                    q.data_ptr(), n, max_len, cells.data_ptr(), info.data_ptr(), self._stream()), self._ctx)
        return cells, info.to(torch.int64) & 0xFFFFFFFF

    # -- connected regions (include/sage_gs.h sgs_regions_label) -----------------------------------------------------------------------
    def label_regions(self, src: torch.Tensor, *, source: Optional[str] = None, lo: int = 1, hi: Optional[int] = None, connectivity: int = 8,
                      max_regions: int = 1024):
        """The connected regions of the set lo <= v <= hi of grids on the device, a whole batch in one call: (labels, rows, counts).
        src: a mask (uint8 or bool; hi defaults to 255, so lo = 1 is "non-zero") or a d2 map (int32 as clearance_map returns it; hi
        defaults to 2^32 - 1, so lo = max_d2 + 1 is "where the agent can stand"), [ny,nx] or [B,ny,nx]; source ("mask" / "d2") is
        inferred from the dtype.  labels int32 of src's shape: 0 outside the set, otherwise 1 + the number of regions whose least
        raster index is smaller — scipy.ndimage.label's numbering, under connectivity 8 or 4.  rows int32 [max_regions,10] or
        [B,max_regions,10] whose bytes are sgs_region_row (_capi.REGION_ROW_DTYPE): row r describes label r + 1 — area, tight box
        (ends exclusive), the first raster index, the sums of x and y; a region whose label exceeds max_regions has no row, rows
        past the number of regions are empty.  counts int32 [4] or [B,4]: regions found (the true number), cells in the set, the
        largest area, the least label that has it.  max_regions = 0: rows is None.  The scratch is this method's.  Nothing is
        copied to the host; asynchronous on the current stream.  All integer: a map's output does not depend on the batch."""
        if source is None:
            source = "d2" if getattr(src, "dtype", None) == torch.int32 else "mask"
        if source not in ("mask", "d2"):
            raise ValueError(f"unknown source {source!r}: 'mask' or 'd2'")
        kind = _capi.REGIONS_SRC_MASK8 if source == "mask" else _capi.REGIONS_SRC_D2
        maps, batched, b, ny, nx, stride = _maps_arg(src, self.device, torch.uint8 if source == "mask" else torch.int32, 1, "src")
        top = 255 if source == "mask" else 0xFFFFFFFF
        hi = top if hi is None else int(hi)
        lo, max_regions = int(lo), int(max_regions)
        if not 0 <= lo <= hi <= top:
            raise ValueError(f"0 <= lo <= hi <= {top} for a {source} source")
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8")
        words = int(self._lib.sgs_regions_work_words(nx, ny, b))
        if words < 0 or max_regions < 0:
            raise ValueError(f"{b} maps of {nx} x {ny} cells, max_regions = {max_regions}: outside what sgs_regions_label takes")
        labels = torch.empty((b, ny, nx), dtype=torch.int32, device=self.device)
        rows = torch.empty((b, max_regions, _capi.REGION_ROW_WORDS), dtype=torch.int32, device=self.device) if max_regions else None
        counts = torch.empty((b, 4), dtype=torch.int32, device=self.device)
        work = torch.empty((words,), dtype=torch.int32, device=self.device)
        params = _capi.SgsRegionsParams(nx, ny, kind, int(connectivity), lo, hi, 0, 0)
        self._lib.check(self._lib.sgs_regions_label(self._ctx, maps.data_ptr(), b, stride, C.byref(params), work.data_ptr(), labels.data_ptr(),
                                                    rows.data_ptr() if max_regions else None, max_regions, counts.data_ptr(), self._stream()), self._ctx)
        if batched:
            return labels, rows, counts
        return labels[0], None if rows is None else rows[0], counts[0]

    def endpoints(self, src: torch.Tensor, items, queries, *, source: Optional[str] = None, max_d2: int = 0, max_dist: int = 50):
        """For every query the free cell nearest to an item's boundary on the side that faces a target (sgs_endpoints): (item_rows,
        query_rows, counts).  src: one map on the device, a mask (uint8 or bool, free iff 0) or a d2 map (int32 as clearance_map
        returns it, free iff d2 > max_d2); source ("mask" / "d2") is inferred from the dtype.  items: (offsets, cells), the CSR of the
        items — int32 tensors on the device or anything np.asarray takes; offsets [n_items + 1], cells raster indices y * nx + x,
        duplicates allowed.  queries: [n, 4] rows of (item, tx, ty, flags), flags bit 0: the target (tx, ty) is given.  item_rows
        int32 [n_items, 14] whose bytes are sgs_endpoints_item (_capi.ENDPOINTS_ITEM_DTYPE), query_rows int32 [n, 4] = (x, y, d,
        n_at_d) or (-1, -1, -1, 0), counts int64 [4]: answered, none, flagged items, bytes of scratch used.  The scratch is this
        method's: a first guess from max_dist, and when the library reports that it needs more (counts[3], one read back), the call
        is made again with that much.  All integer: an answer does not depend on the batch."""
        if source is None:
            source = "d2" if getattr(src, "dtype", None) == torch.int32 else "mask"
        if source not in ("mask", "d2"):
            raise ValueError(f"unknown source {source!r}: 'mask' or 'd2'")
        kind = _capi.ENDPOINTS_SRC_MASK8 if source == "mask" else _capi.ENDPOINTS_SRC_D2
        maps, batched, b, ny, nx, _ = _maps_arg(src, self.device, torch.uint8 if source == "mask" else torch.int32, 1, "src")
        if batched:
            raise ValueError("src must be one map [ny,nx]")
        max_d2, max_dist = int(max_d2), int(max_dist)
        if not 0 <= max_dist <= _capi.ENDPOINTS_MAX_DIST or not 0 <= max_d2 <= 0xFFFFFFFF or (source == "mask" and max_d2 != 0):
            raise ValueError(f"0 <= max_dist <= {_capi.ENDPOINTS_MAX_DIST}; max_d2 is a d2 source's and fits 32 bits")
        offsets, cells = items
        offsets = _flat_i32(offsets, self.device, "item offsets")
        cells = _flat_i32(cells, self.device, "item cells")
        n_items = int(offsets.shape[0]) - 1
        bound = int(self._lib.sgs_endpoints_work_bytes(nx, ny, n_items))
        if bound < 0:
            raise ValueError(f"{n_items} items on {nx} x {ny} cells: outside what sgs_endpoints takes")
        q = _rows_arg(queries, self.device, torch.int32, 4, "queries") if (isinstance(queries, torch.Tensor) or len(queries)) else None
        n_q = 0 if q is None else int(q.shape[0])
        if n_q > _capi.ENDPOINTS_MAX_QUERIES:
            raise ValueError(f"at most {_capi.ENDPOINTS_MAX_QUERIES} queries a call")
        item_rows = torch.empty((n_items, 14), dtype=torch.int32, device=self.device)
        query_rows = torch.empty((n_q, 4), dtype=torch.int32, device=self.device)
        counts = torch.empty((4,), dtype=torch.int64, device=self.device)
        params = _capi.SgsEndpointsParams(nx, ny, kind, max_d2, max_dist, 0, 0)
        side = 2 * max_dist + 16                                                     # a window of a 16 x 16 item
        want = min(bound, 8 * n_items + n_items * min(side, nx) * min(side, ny) + 8)
        for _ in range(2):
            work = torch.empty(((want + 7) // 8,), dtype=torch.int64, device=self.device)
            self._lib.check(self._lib.sgs_endpoints(self._ctx, maps.data_ptr(), C.byref(params), offsets.data_ptr(), cells.data_ptr(), n_items,
                                                    q.data_ptr() if n_q else None, n_q, work.data_ptr(), 8 * int(work.shape[0]), item_rows.data_ptr(),
                                                    query_rows.data_ptr() if n_q else None, counts.data_ptr(), self._stream()), self._ctx)
            need = int(counts[3].item())
            if need <= 8 * int(work.shape[0]):
                break
            want = need
        return item_rows, query_rows, counts

    def set_mesh_record_capacity(self, n: int):
        """Records (triangle, tile) the mesh path's buffer holds to start with (sgs_mesh_set_record_capacity); frames grow it as needed."""
        self._lib.check(self._lib.sgs_mesh_set_record_capacity(self._ctx, int(n)), self._ctx)

    def set_record_capacity(self, n: int):
        self._lib.check(self._lib.sgs_set_record_capacity(self._ctx, int(n)), self._ctx)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.sgs_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostFrames:
    """`depth` pinned uint8 host buffers + device twins of one shape, a D2H copy stream and one event per buffer.
    submit(rgb) packs fp32 -> uint8 RGBA on the CURRENT stream and starts the copy into the next pinned buffer on the copy
    stream (behind an event), so that the copy of frame i overlaps whatever the current stream does next (the rendering of
    frame i+1); wait() on the returned handle blocks until THAT copy has landed and returns the numpy view."""

    class Handle:
        def __init__(self, ring, k, n):
            self._ring, self._k, self._n = ring, k, n

        def wait(self) -> np.ndarray:
            self._ring._done[self._k].synchronize()
            a = self._ring._host_np[self._k]
            return a if self._n is None else a[:self._n]

    def __init__(self, renderer: "Renderer", shape, depth: int):
        self._r, self.shape, self.depth = renderer, tuple(shape), int(depth)
        dev = renderer.device
        self._dev = [torch.empty(self.shape, dtype=torch.uint8, device=dev) for _ in range(self.depth)]
        self._host = [torch.empty(self.shape, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self._host_np = [t.numpy() for t in self._host]
        self._packed = [torch.cuda.Event() for _ in range(self.depth)]
        self._done = [torch.cuda.Event() for _ in range(self.depth)]
        self._copy_stream = torch.cuda.Stream(device=dev)
        self._turn = 0
        self._rgb = None

    def rgb_scratch(self) -> torch.Tensor:
        """An fp32 [..., 3] device buffer of the ring's image shape to render into (one: the pack consumes it in stream order)."""
        if self._rgb is None:
            self._rgb = torch.zeros(self.shape[:-1] + (3,), dtype=torch.float32, device=self._r.device)
        return self._rgb

    def submit(self, rgb: torch.Tensor, tonemap: Optional[str] = None, n: Optional[int] = None, direct: bool = False) -> "HostFrames.Handle":
        """rgb: fp32 [..., 3] of the ring's image shape (a batch [B,H,W,3] counts as one tall image).  n: leading entries that are
        valid (a partial last batch).
        direct=True: the pack kernel writes the PINNED buffer itself, over the link, on the current stream — no device twin, no copy
        engine, no second stream: for ONE frame somebody is waiting for (get_rgba(): 640x480 0.366 -> 0.339 ms, 1024x768 0.418 -> 0.387,
        profiles/r06u); a sweep's batches keep the copy stream, whose transfer runs beside the next batch's kernels."""
        k = self._turn
        self._turn = (k + 1) % self.depth
        self._done[k].synchronize()                  # the buffer's previous copy (depth frames ago) has long landed
        flat = rgb.reshape(-1, rgb.shape[-2], 3)
        if direct:
            if tonemap is not None:
                if tonemap != "reinhard":
                    raise ValueError("tonemap must be None or 'reinhard'")
                flat = flat / (1.0 + flat.clamp_min(0.0))
            r = self._r
            r._lib.check(r._lib.sgs_pack_rgba8(r._ctx, flat.contiguous().data_ptr(), self._host[k].data_ptr(), int(flat.shape[1]), int(flat.shape[0]),
                                               r._stream()), r._ctx)
            self._done[k].record(torch.cuda.current_stream(r.device))
            return HostFrames.Handle(self, k, n)
        self._r.pack_rgba8(flat, tonemap=tonemap, out=self._dev[k].reshape(-1, rgb.shape[-2], 4))
        cur = torch.cuda.current_stream(self._r.device)
        self._packed[k].record(cur)
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(self._packed[k])
            self._host[k].copy_(self._dev[k], non_blocking=True)
            self._done[k].record(self._copy_stream)
        return HostFrames.Handle(self, k, n)


class JpegFrames:
    """`depth` slots of (device byte buffer, pinned byte buffer, pinned offsets / sizes), a copy stream and events.
    submit(rgb, n) encodes the first n frames on the CURRENT stream (sgs_encode_jpeg, asynchronous) and returns a handle; wait() on it
    blocks the host until THAT encode is done, copies only the bytes the files take into the slot's pinned buffer on the copy stream,
    waits for the copy and returns one memoryview per frame, valid until the slot comes round again (depth submits later).  The copy
    overlaps only GPU work that was enqueued BEFORE wait() was called: a caller that wants the pipeline enqueues the next chunk's
    rendering first and waits for this chunk afterwards, as sweep.run does.  rgb must stay as it is until wait() has returned: should the files not fit the
    slot (it starts at a byte a pixel), wait() grows it and encodes them again."""

    class Handle:
        def __init__(self, ring, k, rgb, n):
            self._ring, self._k, self._rgb, self._n = ring, k, rgb, n

        def wait(self, copy: bool = False) -> list:
            ring, k, n = self._ring, self._k, self._n
            if n == 0:
                return []
            ring._encoded[k].synchronize()
            meta = ring._meta[k]
            total = int(meta[0, n - 1]) + int(meta[1, n - 1])
            if total > ring._dev[k].numel():                                  # rare: the chunk is encoded again into a slot that fits
                ring._grow(k, total)
                ring._r._encode_jpeg_into(self._rgb, n, ring._params, ring._dev[k], meta)
                ring._encoded[k].record(torch.cuda.current_stream(ring._r.device))
                ring._encoded[k].synchronize()
            with torch.cuda.stream(ring._copy_stream):
                ring._host[k][:total].copy_(ring._dev[k][:total], non_blocking=True)
            ring._copy_stream.synchronize()
            self._rgb = None
            view = memoryview(ring._host_np[k])
            files = [view[int(o):int(o) + int(z)] for o, z in zip(meta[0, :n].tolist(), meta[1, :n].tolist())]
            return [bytes(f) for f in files] if copy else files

    def __init__(self, renderer: "Renderer", shape, quality: int, subsampling: str, depth: int):
        self._r, self.shape, self.depth = renderer, tuple(shape), int(depth)
        self._params = _capi.jpeg_params(quality, subsampling)
        if not 1 <= self._params.quality <= 100:
            raise ValueError("quality must be in 1..100")
        cap = self.shape[0] * max(1 << 16, self.shape[1] * self.shape[2])
        self._dev, self._host, self._host_np = [None] * self.depth, [None] * self.depth, [None] * self.depth
        for k in range(self.depth):
            self._grow(k, cap)
        self._meta = [torch.zeros((2, self.shape[0]), dtype=torch.int64, pin_memory=True) for _ in range(self.depth)]
        self._encoded = [torch.cuda.Event() for _ in range(self.depth)]
        self._copy_stream = torch.cuda.Stream(device=renderer.device)
        self._turn = 0

    def _grow(self, k, cap):
        self._dev[k] = torch.empty((int(cap),), dtype=torch.uint8, device=self._r.device)
        self._host[k] = torch.empty((int(cap),), dtype=torch.uint8, pin_memory=True)
        self._host_np[k] = self._host[k].numpy()

    def submit(self, rgb: torch.Tensor, n: Optional[int] = None) -> "JpegFrames.Handle":
        rgb, _ = _frames_arg(rgb, self._r.device, torch.float32, (None, None, 3), "rgb")
        n = int(rgb.shape[0]) if n is None else int(n)
        if not 0 <= n <= min(int(rgb.shape[0]), self.shape[0]) or tuple(rgb.shape[1:3]) != self.shape[1:3]:
            raise ValueError(f"the ring holds up to {self.shape[0]} frames of {self.shape[1]} x {self.shape[2]} pixels")
        k = self._turn
        self._turn = (k + 1) % self.depth
        if n:
            self._r._encode_jpeg_into(rgb, n, self._params, self._dev[k], self._meta[k])
            self._encoded[k].record(torch.cuda.current_stream(self._r.device))
        return JpegFrames.Handle(self, k, rgb, n)


_default = {}


def default_renderer(device=None) -> Renderer:
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _default:
        _default[key] = Renderer(torch.device("cuda", key))
    return _default[key]


def render(camera: Camera, gaussians, *, config: Optional[RenderConfig] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The drop-in call surface named by BASELINE.json: one frame, float32 [H,W,3] on the scene's GPU."""
    if isinstance(gaussians, Scene):             # an uploaded scene is drawn by the renderer (GPU) that holds it
        return gaussians._r.render(camera, gaussians, config=config, out=out)
    dev = gaussians.means.device if isinstance(gaussians, Gaussians) else None
    if dev is not None and dev.type != "cuda":
        dev = None
    return default_renderer(dev).render(camera, gaussians, config=config, out=out)
