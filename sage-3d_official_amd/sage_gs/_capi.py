"""ctypes binding of include/sage_gs.h — plain pointers and PODs, no torch.

The product loads exactly one library: ``sage-3d_official_amd/lib/libsage_gs.so`` (built by
``__graft_entry__.build()`` with hipcc for gfx950).  If it is missing, import of the renderer fails
loudly; there is no CPU fallback behind this binding.
"""
from __future__ import annotations

import ctypes as C
import os

SH_DECODE = {"bin_centre": 3, "linear255": 1, "bin_centre_ends": 2}      # include/sage_gs.h SGS_SH_DECODE_* (0 = unspecified: refused at degree > 0)
ABI_VERSION = 114        # include/sage_gs.h SGS_VERSION this binding restates; Lib() refuses any other library
NUM_STAGES = 4
STAGE_NAMES = ("preprocess", "count", "emit", "render")

FLAG_ASYNC, FLAG_TIMING, FLAG_STATS, FLAG_FULL_SORT, FLAG_PIPELINED, FLAG_LOOSE_CULL, FLAG_NO_CHUNK_CULL = 1, 2, 4, 8, 16, 32, 64
FLAG_NO_DEEP = 256
FLAG_NO_FINE_TILES = 512
BACKEND_CPU, BACKEND_HIP = 0, 1
ID_NONE = -1             # include/sage_gs.h SGS_ID_NONE: sgs_render_mesh_ids* where nothing is hit
BUF_TILE_OFFSETS, BUF_SORTED_SLOTS, BUF_SLOT_IDS, BUF_SPLATS, BUF_CHUNK_SKIPPED, BUF_SCENE_GEOM, BUF_SCENE_SH = 0, 1, 2, 3, 4, 5, 6
BUF_SCENE_PERM, BUF_CHUNK_BOUNDS = 7, 8       # the upload's results: uint32 [N] layout position -> original index; float [ceil(N/64), 8]

ERR_NAMES = {-1: "SGS_ERR_INVALID", -2: "SGS_ERR_HIP", -3: "SGS_ERR_OOM", -4: "SGS_ERR_OVERFLOW",
             -5: "SGS_ERR_BACKEND"}

DEFAULT_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib",
                           "libsage_gs.so")

# every symbol include/sage_gs.h declares (tests/test_abi.py checks the built library exports them)
EXPORTS = ("sgs_version", "sgs_struct_sizes", "sgs_config_default", "sgs_create", "sgs_destroy", "sgs_last_error",
           "sgs_set_record_capacity", "sgs_scene_upload", "sgs_scene_upload_compressed", "sgs_scene_free", "sgs_render",
           "sgs_render_rgbd", "sgs_render_batch", "sgs_render_batch_strided", "sgs_frame_sync", "sgs_row_records", "sgs_pack_rgba8", "sgs_debug_read",
           "sgs_tuning_default", "sgs_set_tuning", "sgs_get_tuning",
           "sgs_mesh_upload", "sgs_mesh_free", "sgs_mesh_set_record_capacity", "sgs_render_mesh_depth", "sgs_render_mesh_depth_batch",
           "sgs_mesh_set_labels", "sgs_render_mesh_ids", "sgs_render_mesh_ids_batch",
           "sgs_jpeg_params_default", "sgs_jpeg_bound", "sgs_encode_jpeg", "sgs_jpeg_status",
           "sgs_png_params_default", "sgs_png_bound", "sgs_encode_png", "sgs_png_status",
           "sgs_resize_params_default", "sgs_resize", "sgs_object_table", "sgs_image_similarity",
           "sgs_topdown_params_default", "sgs_topdown_map", "sgs_topdown_summary",
           "sgs_clearance_map", "sgs_clearance_query",
           "sgs_geodesic_tile", "sgs_geodesic_state_words", "sgs_geodesic_field", "sgs_geodesic_path",
           "sgs_regions_tile", "sgs_regions_work_words", "sgs_regions_label",
           "sgs_endpoints_tile", "sgs_endpoints_work_bytes", "sgs_endpoints")


class SgsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class SgsCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("view", C.c_float * 16)]


class SgsConfig(C.Structure):
    _fields_ = [("near_z", C.c_float), ("far_z", C.c_float), ("dilation", C.c_float),
                ("clamp", C.c_float), ("alpha_min", C.c_float), ("alpha_max", C.c_float),
                ("t_min", C.c_float), ("bg", C.c_float * 3), ("sh_degree", C.c_int32),
                ("flags", C.c_uint32), ("tile_row_stride", C.c_int32), ("tile_row_phase", C.c_int32)]


class SgsCompressedScene(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_chunks", C.c_int64), ("sh_degree", C.c_int32), ("sh_decode", C.c_int32),
                ("chunks", C.c_void_p), ("packed", C.c_void_p), ("sh", C.c_void_p)]


class SgsTuning(C.Structure):
    """include/sage_gs.h sgs_tuning: the library's whole tuning surface (it reads nothing from the environment)."""
    _fields_ = [("lanes", C.c_int32), ("group", C.c_int32), ("group_lanes", C.c_int32), ("morton", C.c_int32),
                ("record_capacity", C.c_int64), ("fine_tile_pixels", C.c_int64), ("fine_tile_growth", C.c_double)]


JPEG_420, JPEG_444 = 0, 1
JPEG_SUBSAMPLING = {"4:2:0": JPEG_420, "4:4:4": JPEG_444}


class SgsJpegParams(C.Structure):
    """include/sage_gs.h sgs_jpeg_params."""
    _fields_ = [("quality", C.c_int32), ("subsampling", C.c_int32), ("flags", C.c_uint32), ("reserved_", C.c_int32)]


def jpeg_params(quality=95, subsampling="4:2:0"):
    """sgs_jpeg_params of a quality and a subsampling given as "4:2:0" / "4:4:4" (or SGS_JPEG_* itself)."""
    if isinstance(subsampling, str):
        if subsampling not in JPEG_SUBSAMPLING:
            raise ValueError("subsampling must be '4:2:0' or '4:4:4'")
        subsampling = JPEG_SUBSAMPLING[subsampling]
    return SgsJpegParams(int(quality), int(subsampling), 0, 0)


PNG_RGB8, PNG_DEPTH16 = 0, 1
PNG_FORMAT = {"rgb8": PNG_RGB8, "depth16": PNG_DEPTH16}


class SgsPngParams(C.Structure):
    """include/sage_gs.h sgs_png_params."""
    _fields_ = [("format", C.c_int32), ("depth_scale", C.c_float), ("depth_max", C.c_float), ("reserved", C.c_int32)]


def png_params(format="rgb8", depth_scale=10000.0, depth_max=6.5):
    """sgs_png_params of a format given as "rgb8" / "depth16" (or SGS_PNG_* itself)."""
    if isinstance(format, str):
        if format not in PNG_FORMAT:
            raise ValueError("format must be 'rgb8' or 'depth16'")
        format = PNG_FORMAT[format]
    return SgsPngParams(int(format), float(depth_scale), float(depth_max), 0)


RESIZE_RGB8, RESIZE_F32 = 0, 1
RESIZE_FORMAT = {"rgb8": RESIZE_RGB8, "f32": RESIZE_F32}
RESIZE_BICUBIC, RESIZE_LINEAR = 0, 1
RESIZE_FILTER = {"bicubic": RESIZE_BICUBIC, "linear": RESIZE_LINEAR}


class SgsResizeParams(C.Structure):
    """include/sage_gs.h sgs_resize_params."""
    _fields_ = [("format", C.c_int32), ("filter", C.c_int32), ("dst_width", C.c_int32), ("dst_height", C.c_int32),
                ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("reserved", C.c_int32 * 2)]


def resize_params(format="rgb8", filter="bicubic", dst_width=320, dst_height=240, clip_lo=float("-inf"), clip_hi=float("inf")):
    """sgs_resize_params of a format given as "rgb8" / "f32" and a filter given as "bicubic" / "linear" (or SGS_RESIZE_* themselves)."""
    if isinstance(format, str):
        if format not in RESIZE_FORMAT:
            raise ValueError("format must be 'rgb8' or 'f32'")
        format = RESIZE_FORMAT[format]
    if isinstance(filter, str):
        if filter not in RESIZE_FILTER:
            raise ValueError("filter must be 'bicubic' or 'linear'")
        filter = RESIZE_FILTER[filter]
    return SgsResizeParams(int(format), int(filter), int(dst_width), int(dst_height), float(clip_lo), float(clip_hi))


class SgsObjectRow(C.Structure):
    """include/sage_gs.h sgs_object_row: row k of a frame's visible-object table describes label k."""
    _fields_ = [("n_pixels", C.c_uint32), ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_end", C.c_int32), ("y_end", C.c_int32),
                ("z_min", C.c_float), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64)]


def _object_row_dtype():
    import numpy as np
    return np.dtype([("n_pixels", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("z_min", "<f4"),
                     ("sum_x", "<u8"), ("sum_y", "<u8")])


OBJECT_ROW_DTYPE = _object_row_dtype()       # the same 40 bytes as a NumPy record: ten int32 words of Renderer.object_table's rows
OBJECT_ROW_WORDS = 10
VISIBLE_OBJECT_DTYPE = __import__("numpy").dtype([("label", "<i4")] + [(n, OBJECT_ROW_DTYPE.fields[n][0]) for n in OBJECT_ROW_DTYPE.names])
assert OBJECT_ROW_DTYPE.itemsize == C.sizeof(SgsObjectRow) == 4 * OBJECT_ROW_WORDS


class SgsSimilarityRow(C.Structure):
    """include/sage_gs.h sgs_similarity_row: one frame's sums against its target."""
    _fields_ = [("ssim_q", C.c_int64 * 3), ("sse", C.c_uint64 * 3), ("n_windows", C.c_uint64), ("n_pixels", C.c_uint64)]


SIMILARITY_ROW_DTYPE = __import__("numpy").dtype([("ssim_q", "<i8", (3,)), ("sse", "<u8", (3,)), ("n_windows", "<u8"), ("n_pixels", "<u8")])
SIMILARITY_Q_BITS = 30                       # fractional bits of ssim_q
SIMILARITY_WINDOW, SIMILARITY_TILE_W, SIMILARITY_TILE_H = 11, 32, 32      # include/sage_gs.h SGS_SIM_WINDOW, SGS_SIM_TILE_W, SGS_SIM_TILE_H
# Renderer.image_similarity's record: the raw row, then the host divisions
SIMILARITY_DTYPE = __import__("numpy").dtype(SIMILARITY_ROW_DTYPE.descr + [("ssim", "<f8"), ("ssim_rgb", "<f8", (3,)), ("mse", "<f8"), ("psnr", "<f8")])
assert SIMILARITY_ROW_DTYPE.itemsize == C.sizeof(SgsSimilarityRow) == 64


TOPDOWN_CLEAR = 1                            # include/sage_gs.h SGS_TOPDOWN_CLEAR (sgs_topdown_params.flags)


class SgsTopdownParams(C.Structure):
    """include/sage_gs.h sgs_topdown_params: the grid, the depth range and the two height bands of the top-down seen map."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("origin_x", C.c_float), ("origin_y", C.c_float), ("cell_size", C.c_float),
                ("min_z", C.c_float), ("max_z", C.c_float), ("free_lo", C.c_float), ("free_hi", C.c_float),
                ("occ_lo", C.c_float), ("occ_hi", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32)]


class SgsTopdownSummary(C.Structure):
    """sgs_topdown_summary's out: uint64[4]."""
    _fields_ = [("occupied_cells", C.c_uint64), ("free_cells", C.c_uint64), ("free_hits", C.c_uint64), ("occupied_hits", C.c_uint64)]


assert C.sizeof(SgsTopdownParams) == 52 and C.sizeof(SgsTopdownSummary) == 32


CLEARANCE_NONE = 0xFFFFFFFF                  # include/sage_gs.h SGS_CLEARANCE_NONE: d2 of a map without obstacles
CLEARANCE_SRC_MASK8, CLEARANCE_SRC_TOPDOWN = 0, 1
CLEARANCE_UNSEEN_BLOCKS = 1                  # sgs_clearance_params.flags
CLEARANCE_NEGATE, CLEARANCE_FLIP_X, CLEARANCE_FLIP_Y = 1, 2, 4       # sgs_clearance_frame.flags


class SgsClearanceParams(C.Structure):
    """include/sage_gs.h sgs_clearance_params: the map's size, what its source is and where its counters are cut."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("source", C.c_int32), ("flags", C.c_uint32), ("min_hits", C.c_uint32),
                ("max_d2", C.c_uint32), ("reserved", C.c_int32)]


class SgsClearanceFrame(C.Structure):
    """include/sage_gs.h sgs_clearance_frame: how sgs_clearance_query takes a caller's coordinates to a pixel of the map."""
    _fields_ = [("min_x", C.c_double), ("min_y", C.c_double), ("sum_x", C.c_double), ("sum_y", C.c_double), ("scale", C.c_double),
                ("flags", C.c_uint32), ("margin", C.c_int32), ("max_d2", C.c_uint32), ("n_samples", C.c_int32), ("reserved", C.c_int64)]


# the struct-size handshake of the two: the library asserts the same figures when it is compiled (csrc/sgs_api.hip)
assert C.sizeof(SgsClearanceParams) == 28 and C.sizeof(SgsClearanceFrame) == 64 and SgsClearanceFrame.reserved.offset == 56


GEODESIC_NONE = 0xFFFFFFFF                   # include/sage_gs.h SGS_GEODESIC_NONE: both words of a blocked or unreachable cell
GEODESIC_SRC_MASK8, GEODESIC_SRC_D2 = 0, 1
GEODESIC_CONTINUE = 1                        # sgs_geodesic_params.flags
GEODESIC_MAX_N, GEODESIC_MAX_FIELDS, GEODESIC_PATH_MAX_FIELDS = 4096, 65535, 512
GEODESIC_PATH_OK, GEODESIC_PATH_UNREACHABLE, GEODESIC_PATH_TRUNCATED, GEODESIC_PATH_INVALID, GEODESIC_PATH_NOT_FINAL = 0, 1, 2, 3, 4


class SgsGeodesicParams(C.Structure):
    """include/sage_gs.h sgs_geodesic_params: the map's size, what its source is, and whether a field call continues an earlier one."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("source", C.c_int32), ("max_d2", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_int32)]


assert C.sizeof(SgsGeodesicParams) == 24


REGIONS_SRC_MASK8, REGIONS_SRC_D2 = 0, 1     # include/sage_gs.h SGS_REGIONS_SRC_*
REGIONS_MAX_N, REGIONS_MAX_MAPS = 4096, 65535
REGIONS_NO_FIRST = 0xFFFFFFFF                # sgs_region_row.first of an empty row


class SgsRegionsParams(C.Structure):
    """include/sage_gs.h sgs_regions_params: the map's size, what its source is, the connectivity and the set lo <= v <= hi."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("source", C.c_int32), ("connectivity", C.c_int32), ("lo", C.c_uint32),
                ("hi", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


class SgsRegionRow(C.Structure):
    """include/sage_gs.h sgs_region_row: row r of a map's region table describes label r + 1."""
    _fields_ = [("area", C.c_uint32), ("x_min", C.c_int32), ("y_min", C.c_int32), ("x_end", C.c_int32), ("y_end", C.c_int32),
                ("first", C.c_uint32), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64)]


# the same 40 bytes as a NumPy record: ten int32 words of Renderer.label_regions' rows
REGION_ROW_DTYPE = __import__("numpy").dtype([("area", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("first", "<u4"),
                                              ("sum_x", "<u8"), ("sum_y", "<u8")])
REGION_ROW_WORDS = 10
# the struct-size handshake: the library asserts the same figures when it is compiled (csrc/sgs_api.hip)
assert C.sizeof(SgsRegionsParams) == 32 and REGION_ROW_DTYPE.itemsize == C.sizeof(SgsRegionRow) == 4 * REGION_ROW_WORDS


ENDPOINTS_SRC_MASK8, ENDPOINTS_SRC_D2 = 0, 1  # include/sage_gs.h SGS_ENDPOINTS_*
ENDPOINTS_MAX_N, ENDPOINTS_MAX_ITEMS, ENDPOINTS_MAX_DIST, ENDPOINTS_MAX_ENTRIES, ENDPOINTS_MAX_QUERIES = 4096, 65535, 63, 1 << 19, 1 << 22
ENDPOINTS_ITEM_EMPTY, ENDPOINTS_ITEM_BAD_CELL, ENDPOINTS_ITEM_TOO_LONG = 1, 2, 4
ENDPOINTS_QUERY_TOWARDS = 1


class SgsEndpointsParams(C.Structure):
    """include/sage_gs.h sgs_endpoints_params: the grid's size, what its source is, the free limit of a d2 map and the search distance."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("source", C.c_int32), ("max_d2", C.c_uint32), ("max_dist", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_int32)]


# the three row types as NumPy records: sgs_endpoints_item (56 bytes), sgs_endpoints_query and sgs_endpoints_answer (16 bytes each)
ENDPOINTS_ITEM_DTYPE = __import__("numpy").dtype([("n", "<u4"), ("flags", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"),
                                                  ("cx", "<i4"), ("cy", "<i4"), ("boundary", "<u4"), ("reserved", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8")])
ENDPOINTS_QUERY_DTYPE = __import__("numpy").dtype([("item", "<i4"), ("tx", "<i4"), ("ty", "<i4"), ("flags", "<u4")])
ENDPOINTS_ANSWER_DTYPE = __import__("numpy").dtype([("x", "<i4"), ("y", "<i4"), ("d", "<i4"), ("n_at_d", "<i4")])
assert C.sizeof(SgsEndpointsParams) == 28 and ENDPOINTS_ITEM_DTYPE.itemsize == 56 and ENDPOINTS_QUERY_DTYPE.itemsize == ENDPOINTS_ANSWER_DTYPE.itemsize == 16


class SgsStats(C.Structure):
    _fields_ = [("n_gaussians", C.c_int64), ("n_visible", C.c_int64), ("d_total", C.c_int64),
                ("d_fetched", C.c_int64), ("n_pixels", C.c_int64), ("n_tiles", C.c_int32),
                ("max_tile_len", C.c_int32), ("n_spill_tiles", C.c_int32), ("retries", C.c_int32),
                ("ms", C.c_float * NUM_STAGES), ("ms_total", C.c_float),
                ("bytes", C.c_int64 * NUM_STAGES), ("d_super", C.c_int64), ("n_deep_windows", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("ms", "bytes")}
        d["ms"] = {n: float(self.ms[i]) for i, n in enumerate(STAGE_NAMES)}
        d["bytes"] = {n: int(self.bytes[i]) for i, n in enumerate(STAGE_NAMES)}
        return d


class Lib:
    """A loaded libsage_gs.so with typed entry points."""

    def __init__(self, path=None):
        path = path or os.environ.get("SAGE_GS_LIB") or DEFAULT_LIB
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C sage-3d_official_amd). There is no CPU fallback.")
        self.path = path
        # One HIP runtime per process: libsage_gs.so needs libamdhip64.so.7, and PyTorch ships its own
        # copy under the same SONAME.  Importing torch FIRST makes the loader hand that already-loaded
        # copy to our library, so device pointers and streams are shared with torch (loading ours first
        # pulls /opt/rocm's copy in and the second runtime then finds no device).
        import torch  # noqa: F401
        lib = self._lib = C.CDLL(path)
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
        lib.sgs_version.restype = i32
        # the structs below are restated by hand: a library built from another header (other sizes / strides) would write past
        # them silently, so the binding refuses it here — before any call that takes a struct
        if int(lib.sgs_version()) != ABI_VERSION:
            raise ImportError(f"{path} reports ABI version {int(lib.sgs_version())}, this binding is written for {ABI_VERSION}: "
                              "rebuild the library (make -C sage-3d_official_amd) or update sage_gs")
        lib.sgs_struct_sizes.argtypes = [C.POINTER(C.c_int32)] * 3; lib.sgs_struct_sizes.restype = None
        sz = (C.c_int32 * 3)()
        lib.sgs_struct_sizes(C.cast(C.byref(sz, 0), C.POINTER(C.c_int32)), C.cast(C.byref(sz, 4), C.POINTER(C.c_int32)),
                             C.cast(C.byref(sz, 8), C.POINTER(C.c_int32)))
        mine = (C.sizeof(SgsCamera), C.sizeof(SgsConfig), C.sizeof(SgsStats))
        if tuple(sz) != mine:
            raise ImportError(f"{path}: struct sizes (camera, config, stats) = {tuple(sz)}, this binding's = {mine}")
        lib.sgs_config_default.argtypes = [C.POINTER(SgsConfig)]; lib.sgs_config_default.restype = None
        lib.sgs_create.argtypes = [i32, i32, C.POINTER(vp)]
        lib.sgs_destroy.argtypes = [vp]
        lib.sgs_last_error.argtypes = [vp]; lib.sgs_last_error.restype = C.c_char_p
        lib.sgs_set_record_capacity.argtypes = [vp, i64]
        lib.sgs_scene_upload.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        lib.sgs_scene_upload_compressed.argtypes = [vp, C.POINTER(SgsCompressedScene), i32, C.POINTER(vp)]
        lib.sgs_scene_free.argtypes = [vp, vp]
        lib.sgs_render.argtypes = [vp, vp, C.POINTER(SgsCamera), C.POINTER(SgsConfig), i32, i32, vp,
                                   C.POINTER(SgsStats), vp]
        lib.sgs_render_rgbd.argtypes = [vp, vp, C.POINTER(SgsCamera), C.POINTER(SgsConfig), i32, i32, vp, vp,
                                        C.POINTER(SgsStats), vp]
        lib.sgs_render_batch.argtypes = [vp, vp, C.POINTER(SgsCamera), i32, C.POINTER(SgsConfig), i32,
                                         i32, vp, C.POINTER(SgsStats), vp]
        lib.sgs_render_batch_strided.argtypes = [vp, vp, C.POINTER(SgsCamera), i32, C.POINTER(SgsConfig), i32,
                                                 i32, vp, i64, C.POINTER(SgsStats), vp]
        lib.sgs_frame_sync.argtypes = [vp, C.POINTER(SgsStats)]
        lib.sgs_row_records.argtypes = [vp, vp, i32, i32]
        lib.sgs_pack_rgba8.argtypes = [vp, vp, vp, i32, i32, vp]
        lib.sgs_debug_read.argtypes = [vp, i32, vp, i64]; lib.sgs_debug_read.restype = i64
        lib.sgs_tuning_default.argtypes = [C.POINTER(SgsTuning)]; lib.sgs_tuning_default.restype = None
        lib.sgs_set_tuning.argtypes = [vp, C.POINTER(SgsTuning)]
        lib.sgs_get_tuning.argtypes = [vp, C.POINTER(SgsTuning)]
        lib.sgs_mesh_upload.argtypes = [vp, i64, vp, i64, vp, i32, C.POINTER(vp)]
        lib.sgs_mesh_free.argtypes = [vp, vp]
        lib.sgs_mesh_set_record_capacity.argtypes = [vp, i64]
        lib.sgs_render_mesh_depth.argtypes = [vp, vp, C.POINTER(SgsCamera), C.POINTER(SgsConfig), i32, i32, vp, C.POINTER(SgsStats), vp]
        lib.sgs_render_mesh_depth_batch.argtypes = [vp, vp, vp, i32, C.POINTER(SgsConfig), vp, vp, vp]
        lib.sgs_mesh_set_labels.argtypes = [vp, vp, vp, i32]
        lib.sgs_render_mesh_ids.argtypes = [vp, vp, C.POINTER(SgsCamera), C.POINTER(SgsConfig), i32, i32, vp, vp, C.POINTER(SgsStats), vp]
        lib.sgs_render_mesh_ids_batch.argtypes = [vp, vp, vp, i32, C.POINTER(SgsConfig), vp, vp, vp, vp]
        lib.sgs_jpeg_params_default.argtypes = [C.POINTER(SgsJpegParams)]; lib.sgs_jpeg_params_default.restype = None
        lib.sgs_jpeg_bound.argtypes = [i32, i32, C.POINTER(SgsJpegParams)]; lib.sgs_jpeg_bound.restype = i64
        lib.sgs_encode_jpeg.argtypes = [vp, vp, i32, i32, i32, i64, C.POINTER(SgsJpegParams), vp, i64, vp, vp, vp]
        lib.sgs_jpeg_status.argtypes = [vp, C.POINTER(i64)]
        lib.sgs_png_params_default.argtypes = [C.POINTER(SgsPngParams)]; lib.sgs_png_params_default.restype = None
        lib.sgs_png_bound.argtypes = [i32, i32, C.POINTER(SgsPngParams)]; lib.sgs_png_bound.restype = i64
        lib.sgs_encode_png.argtypes = [vp, vp, i32, i32, i32, i64, C.POINTER(SgsPngParams), vp, i64, vp, vp, vp]
        lib.sgs_png_status.argtypes = [vp, C.POINTER(i64)]
        lib.sgs_resize_params_default.argtypes = [C.POINTER(SgsResizeParams)]; lib.sgs_resize_params_default.restype = None
        lib.sgs_resize.argtypes = [vp, vp, i32, i32, i32, i64, C.POINTER(SgsResizeParams), vp, i64, vp]
        lib.sgs_object_table.argtypes = [vp, vp, vp, i32, i32, i32, i64, C.c_int32, vp, vp, vp]
        lib.sgs_image_similarity.argtypes = [vp, vp, i32, i32, i32, i64, vp, i64, vp, vp]
        lib.sgs_topdown_params_default.argtypes = [C.POINTER(SgsTopdownParams)]; lib.sgs_topdown_params_default.restype = None
        lib.sgs_topdown_map.argtypes = [vp, vp, i32, i32, i32, i64, vp, C.POINTER(SgsTopdownParams), vp, vp, vp]
        lib.sgs_topdown_summary.argtypes = [vp, vp, i32, i32, C.c_uint32, vp, vp]
        lib.sgs_clearance_map.argtypes = [vp, vp, i32, i64, C.POINTER(SgsClearanceParams), vp, vp, vp, vp]
        lib.sgs_clearance_query.argtypes = [vp, vp, i32, i32, vp, i32, C.POINTER(SgsClearanceFrame), vp, vp]
        lib.sgs_geodesic_tile.argtypes = []
        lib.sgs_geodesic_state_words.argtypes = [i32, i32, i32]; lib.sgs_geodesic_state_words.restype = i64
        lib.sgs_geodesic_field.argtypes = [vp, vp, i32, i64, C.POINTER(SgsGeodesicParams), vp, i32, vp, i32, vp, vp, i32, vp, vp]
        lib.sgs_geodesic_path.argtypes = [vp, vp, i32, i64, C.POINTER(SgsGeodesicParams), vp, i32, vp, vp, i32, i32, vp, vp, vp]
        lib.sgs_regions_tile.argtypes = []
        lib.sgs_regions_work_words.argtypes = [i32, i32, i32]; lib.sgs_regions_work_words.restype = i64
        lib.sgs_regions_label.argtypes = [vp, vp, i32, i64, C.POINTER(SgsRegionsParams), vp, vp, vp, C.c_int32, vp, vp]
        lib.sgs_endpoints_tile.argtypes = []
        lib.sgs_endpoints_work_bytes.argtypes = [i32, i32, i32]; lib.sgs_endpoints_work_bytes.restype = i64
        lib.sgs_endpoints.argtypes = [vp, vp, C.POINTER(SgsEndpointsParams), vp, vp, i32, vp, i32, vp, i64, vp, vp, vp, vp]

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def check(self, rc, ctx=None):
        if rc < 0:
            msg = self._lib.sgs_last_error(ctx)
            raise SgsError(int(rc), (msg or b"").decode("utf-8", "replace"))
        return rc

    def version(self):
        return int(self._lib.sgs_version())

    def default_config(self):
        cfg = SgsConfig()
        self._lib.sgs_config_default(C.byref(cfg))
        return cfg


def make_camera(width, height, fx, fy, cx, cy, view):
    cam = SgsCamera(int(width), int(height), float(fx), float(fy), float(cx), float(cy))
    flat = [float(v) for row in view for v in (row if hasattr(row, "__len__") else [row])]
    if len(flat) != 16:
        raise ValueError("view must be 4x4")
    cam.view[:] = flat                   # (one slice assignment: a loop over the sixteen ctypes elements was 6 us of a 0.3-ms call)
    return cam
