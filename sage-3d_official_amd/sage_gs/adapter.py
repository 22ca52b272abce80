"""`GsCamera` — the Isaac Sim Camera protocol, as far as SAGE-3D's callers use it.

`simple_env.py:840-907,1284,1380` and `generate_images.py:344-350,417-432` construct
`Camera(prim_path, frequency, resolution)`, call `.initialize()`, `.set_world_pose(position, orientation)`
/ `.get_world_pose()`, and read `.get_rgba()` (uint8 [H,W,4]) after stepping the world.  This object
offers the same calls on top of the MI355X renderer, so those loops can be pointed at it unchanged:
there is no world to step — `get_rgba()` renders on demand.  Unlike the reference's callers' expectations
of Isaac Sim, failures raise (no silent `None` / black frames).
"""
from __future__ import annotations

import re
from typing import Optional, Sequence, Tuple

import numpy as np

from . import camera as cam_conv
from .renderer import Camera, RenderConfig, Renderer


# near / far of collision-mesh depth: Isaac Sim's default camera clipping range starts at 0.01 m (below get_depth's 0.1 m clip)
MESH_CONFIG = RenderConfig(near=0.01)


class GsCamera:
    def __init__(self, renderer: Renderer, scene, prim_path: str = "/World/Camera", frequency: int = 30,
                 resolution: Tuple[int, int] = (640, 480), config: Optional[RenderConfig] = None, collision_mesh=None,
                 mesh_config: Optional[RenderConfig] = None, instance_paths: Optional[Sequence[str]] = None,
                 output_size: Optional[Tuple[int, int]] = None, resample: str = "bicubic"):
        """collision_mesh: a Mesh (Renderer.upload_mesh) — get_depth() / get_current_frame()["distance_to_image_plane"] then come
        from it, as the reference's come from /World/scene_collision (simple_env.py:1395-1589); mesh_config: its near / far (default
        MESH_CONFIG).  Without a mesh, depth is the Gaussians' expected depth, as before.
        instance_paths: the prim path of every label of the mesh (mesh.read_usda_mesh(return_prims=True)'s prim_paths, the mesh uploaded
        with labels=tri_prim) — the names of the instance-id channel (get_instance_ids, add_instance_id_segmentation_to_frame).
        output_size=(w, h): the camera still renders at `resolution`, with unchanged intrinsics, and every colour and depth getter
        returns the picture resized on the device (Renderer.resize with `resample`: "bicubic" is PIL's Image.resize((w, h)) bit for
        bit, "linear" bilinear) — what the benchmark's low-res mode makes of each observation on the host
        (run_benchmark.py:1409-1419, 1441-1451); a loop that finds the frame's shape already (h, w) skips its own resize.  Depth is
        clipped on the device, then resized, then not clipped again.  The instance-id channel is NOT resized — ids do not interpolate
        — and keeps the render resolution.  None (default): every method is what it is without the argument."""
        if resample not in ("bicubic", "linear"):
            raise ValueError("resample must be 'bicubic' or 'linear'")
        self._out = None if output_size is None else (int(output_size[0]), int(output_size[1]))
        if self._out is not None and (min(self._out) < 1 or max(self._out) > 65535):
            raise ValueError("output_size must be (width, height) within 1..65535")
        self._resample = resample
        self._r, self._scene, self.prim_path, self.frequency = renderer, scene, prim_path, frequency
        self._mesh = collision_mesh
        self._mesh_config = mesh_config if mesh_config is not None else MESH_CONFIG
        self._instance_paths = None if instance_paths is None else [str(p) for p in instance_paths]
        self._instance_in_frame = False
        self._boxes_in_frame = False
        self._explore = None                                              # start_exploration_map: (TopdownGrid, model_to_map, grid, counts)
        self._target = None                                               # set_target_image: uint8 [h,w,3] on the device, at get_output_size()
        self._w, self._h = int(resolution[0]), int(resolution[1])         # Isaac resolution = (width, height)
        self._pos = np.zeros(3, np.float32)
        self._orient = np.array([1.0, 0.0, 0.0, 0.0], np.float32)         # (w, x, y, z)
        self._focal_over_aperture = cam_conv.REF_FOCAL_OVER_APERTURE      # focalLength 8.0 (simple_env.py:905)
        self._config = config
        self._initialized = False

    # -- the protocol ---------------------------------------------------------------------------------
    def initialize(self):
        self._initialized = True

    def set_world_pose(self, position: Sequence[float] = None, orientation: Sequence[float] = None):
        if position is not None:
            self._pos = np.asarray(position, np.float32).reshape(3).copy()
        if orientation is not None:
            self._orient = np.asarray(orientation, np.float32).reshape(4).copy()

    def get_world_pose(self):
        return self._pos.copy(), self._orient.copy()

    def set_focal_length(self, focal_length_mm: float, horizontal_aperture_mm: float = 20.955):
        self._focal_over_aperture = float(focal_length_mm) / float(horizontal_aperture_mm)

    def get_resolution(self):
        return self._w, self._h

    def get_output_size(self):
        """(width, height) of the pictures the getters return: output_size, or the resolution without one."""
        return self._out if self._out is not None else (self._w, self._h)

    def _resized(self, frames, kind="rgb", clip=None):
        """`frames` as the getters return them: resized to output_size on the device (with one), else unchanged."""
        if self._out is None:
            return frames
        return self._r.resize(frames.contiguous(), self._out, filter=self._resample, kind=kind, clip=clip)

    def _camera(self) -> Camera:
        f = self._w * self._focal_over_aperture
        return Camera(self._w, self._h, f, f, self._w / 2.0, self._h / 2.0,
                      cam_conv.view_from_isaac_pose(self._pos, self._orient))

    def get_rgb_tensor(self):
        """float32 [H,W,3] on the GPU (linear RGB) — for consumers that stay on the device.  With output_size: [h,w,3] on the levels
        k / 255 (Renderer.resize)."""
        return self._resized(self._r.render(self._camera(), self._scene, config=self._config))

    def get_rgba(self, copy: bool = True) -> np.ndarray:
        """uint8 [H,W,4], alpha 255 — what `cam.get_rgba()` returns (simple_env.py:1380; generate_images.py:428).  Render, pack and
        the copy into a PINNED host buffer are one stream-ordered sequence with a single wait (Renderer.render_rgba8_host).

        copy=True (default): a fresh array per call (a 640x480x4 memcpy, ~50 us) — safe for a stereo pair, several cameras on one
        renderer, or a caller that keeps its last N observations.  copy=False: a VIEW of the renderer's pinned ring of depth 2, which all
        cameras of one resolution on this renderer SHARE — the third get_rgba() at that resolution, from any of them, overwrites the
        first; for the reference's own callers, which copy at once (generate_images.py:431 `.copy()`, simple_env.py:1386 `.astype`)."""
        if self._out is None:
            img = self._r.render_rgba8_host(self._camera(), self._scene, config=self._config)
        else:
            img = self._r.render_rgba8_host(self._camera(), self._scene, config=self._config, output_size=self._out, resample=self._resample)
        return img.copy() if copy else img

    # -- similarity to a target picture (Renderer.image_similarity: this project's own definition) ---------------------------------
    def set_target_image(self, img):
        """The picture get_image_similarity() compares the view with: a PIL image, or uint8 [h,w,3] / [h,w,4] (get_rgba()'s; alpha is
        dropped) as a NumPy array or a tensor.  It is brought to get_output_size() ONCE, here, when its size differs — with the
        camera's own resample through Renderer.resize, on the device — and stays there as uint8 levels.  None forgets it.  The goal
        image of an ImgNav episode (task_types.py:183-208)."""
        if img is None:
            self._target = None
            return
        import torch
        if isinstance(img, torch.Tensor):
            img = img.detach().cpu().numpy()
        elif hasattr(img, "convert") and hasattr(img, "size"):
            img = np.asarray(img.convert("RGB"))
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
            raise ValueError("the target image must be uint8 [h,w,3] or [h,w,4]")
        img = np.ascontiguousarray(img[..., :3])
        w, h = self.get_output_size()
        if (img.shape[1], img.shape[0]) == (w, h):
            self._target = torch.from_numpy(img).to(self._r.device)
            return
        frame = torch.from_numpy(img.astype(np.float32) / np.float32(255.0)).to(self._r.device)      # on the levels: k / 255
        resized = self._r.resize(frame, (w, h), filter=self._resample)
        self._target = self._r.pack_rgba8(resized)[..., :3].contiguous()

    def get_image_similarity(self):
        """One record of Renderer.image_similarity (ssim, ssim_rgb, mse, psnr and the exact sums) for the picture get_rgba() would
        show now against the target image: the view is rendered, resized with output_size, and compared on the device."""
        if self._target is None:
            raise RuntimeError("no target image: call set_target_image first")
        return self._r.image_similarity(self.get_rgb_tensor(), self._target)[0]

    def get_jpeg(self, quality: int = 75) -> bytes:
        """The current view as the bytes of a baseline JPEG file — the picture get_rgba() returns, encoded on the GPU
        (Renderer.encode_jpeg): for callers shaped like the VLM client, which JPEG-encodes every observation before it leaves the
        process (vlm_client_modular.py:346-351)."""
        return self._r.encode_jpeg(self.get_rgb_tensor(), quality=quality)[0]

    def get_png(self) -> bytes:
        """The current view as the bytes of an 8-bit RGB PNG file — exactly get_rgba()'s picture, encoded on the GPU
        (Renderer.encode_png): a frame of the episode's frame_%05d.png sequence (simple_env.py:2757-2759)."""
        return self._r.encode_png(self.get_rgb_tensor(), format="rgb8")[0]

    def get_depth_png(self, clip=(0.1, 6.5)) -> bytes:
        """The depth observation as the VLM client sends it (vlm_client_modular.py:355-365): a 16-bit grey PNG of
        np.clip(get_depth(clip), 0, 6.5) * 10000 -> uint16, made on the GPU from the device depth — the fp32 frame does not cross the
        link.  The lower clip bound is applied on the device before the encoder; its upper bound is the encoder's depth_max."""
        import torch
        depth = self._mesh_depth() if self._mesh is not None else self._rgb_depth()[1]
        if self._out is not None:        # clipped as it is loaded, resized, and not clipped again below the encoder's own depth_max
            depth = self._resized(depth, "depth", (float(clip[0]), float(clip[1])))
        else:
            depth = torch.clamp(depth, min=float(clip[0])).contiguous()
        return self._r.encode_png(depth, format="depth16", depth_scale=10000.0, depth_max=float(clip[1]))[0]

    def _mesh_depth(self):
        """depth [H,W] float32 on the GPU: distance to the image plane of the nearest collision-mesh triangle, +inf where none."""
        return self._r.render_mesh_depth(self._camera(), self._mesh, config=self._mesh_config)

    def _rgb_depth(self):
        """(rgb [H,W,3] float32 on the GPU, depth [H,W] float32 on the GPU): depth = the scene's expected view depth along
        the optical axis, sum(T alpha z) / coverage — the Gaussian-scene counterpart of Isaac Sim's
        distance_to_image_plane (which the reference reads off the COLLISION MESH, simple_env.py:1401-1409) — and +inf
        where the pixel's coverage is below 1e-4 (nothing hit: what the simulator reports there)."""
        import torch
        rgb, aux = self._r.render(self._camera(), self._scene, config=self._config, return_aux=True)
        cov = aux[..., 1]
        depth = torch.where(cov > 1.0e-4, aux[..., 0] / cov.clamp_min(1.0e-4), torch.full_like(cov, float("inf")))
        return rgb, depth

    def get_current_frame(self) -> dict:
        """{'rgba': uint8 [H,W,4], 'distance_to_image_plane': float32 [H,W]} (simple_env.py:286,1425,1659).  With output_size both are
        resized; the distance is the simulator's raw one (+inf where nothing is hit) and is resized unclipped: a pixel whose window
        holds such a sample is unspecified (get_depth() clips first, as the reference's get_depth does)."""
        if self._mesh is not None:
            rgb = self._r.render(self._camera(), self._scene, config=self._config)
            depth = self._mesh_depth()
        else:
            rgb, depth = self._rgb_depth()
        frame = {"rgba": self._r.pack_rgba8(self._resized(rgb)).cpu().numpy(), "distance_to_image_plane": self._resized(depth, "depth").cpu().numpy()}
        if self._instance_in_frame:
            frame["instance_id_segmentation"] = self._instance_segmentation()
        if self._boxes_in_frame:
            frame["bounding_box_2d_tight"] = self._bounding_boxes()
        return frame

    # -- instance ids: which object of the collision mesh each pixel shows.  THIS PROJECT'S OWN channel: the reference never reads one
    # (its object-based success decides on the 2-D map), and the dictionary below follows Isaac Sim's instance_id_segmentation
    # annotator only as far as its shape is commonly described — nothing of the reference depends on it.
    def _mesh_ids(self):
        """ids [H,W] int32 on the GPU (Renderer.render_mesh_ids): the label of the nearest collision-mesh triangle, -1 where none."""
        if self._mesh is None:
            raise RuntimeError("instance ids come from the collision mesh: construct the camera with collision_mesh=")
        return self._r.render_mesh_ids(self._camera(), self._mesh, config=self._mesh_config)

    def get_instance_ids(self) -> np.ndarray:
        """int32 [H,W]: per pixel the label of the collision-mesh object in view — the index into instance_paths when the mesh was
        uploaded with labels=tri_prim — and -1 where nothing is hit.  The hit is the one get_depth() reports."""
        return self._mesh_ids().cpu().numpy()

    def add_instance_id_segmentation_to_frame(self):
        """get_current_frame() also returns "instance_id_segmentation" from now on (needs collision_mesh=)."""
        if self._mesh is None:
            raise RuntimeError("instance ids come from the collision mesh: construct the camera with collision_mesh=")
        self._instance_in_frame = True

    def _instance_segmentation(self) -> dict:
        """{"data": uint32 [H,W] = id + 1 (0: nothing hit), "info": {"idToLabels": {"0": "BACKGROUND", str(k + 1): instance_paths[k]}}};
        without instance_paths, the ids in the frame are named "label_<id>"."""
        ids = self.get_instance_ids()
        return {"data": (ids + 1).astype(np.uint32), "info": {"idToLabels": self._id_to_labels(np.unique(ids[ids >= 0]))}}

    def _id_to_labels(self, present) -> dict:
        """idToLabels of a frame that shows the labels `present` (ascending)."""
        if self._instance_paths is not None:
            if len(present) and int(present[-1]) >= len(self._instance_paths):
                raise ValueError(f"the mesh has a label {int(present[-1])}, instance_paths names {len(self._instance_paths)}")
            names = {str(k + 1): p for k, p in enumerate(self._instance_paths)}
        else:
            names = {str(int(k) + 1): f"label_{int(k)}" for k in present}
        return {"0": "BACKGROUND", **names}

    def _visible_rows(self, min_pixels=1):
        """The visible-object rows (Renderer.visible_objects) of ONE render_mesh_ids(return_depth=True) at the render resolution."""
        if self._mesh is None:
            raise RuntimeError("instance ids come from the collision mesh: construct the camera with collision_mesh=")
        ids, depth = self._r.render_mesh_ids(self._camera(), self._mesh, config=self._mesh_config, return_depth=True)
        n = len(self._instance_paths) if self._instance_paths is not None else max(int(ids.max().item()) + 1, 1)
        return self._r.visible_objects(ids, depth, n_labels=n, min_pixels=min_pixels)[0]

    def get_visible_objects(self, min_pixels: int = 1) -> list:
        """Which objects of the collision mesh the view shows, reduced on the GPU from the ids and the depth of one render (only the
        table's rows cross the link): a list, by ascending label, of {"label", "path" (instance_paths[label], or None without
        instance_paths), "pixels", "bbox" (x_min, y_min, x_max, y_max — inclusive), "centre" (mean x, mean y of the object's pixels,
        float64), "nearest_m" (the least distance to the image plane among them)} for every label that covers at least min_pixels
        pixels.  Ids are never resized: the figures are in pixels of the render resolution, whatever output_size is.  Needs
        collision_mesh=.  This project's own observation (the reference reads none like it); a label instance_paths does not name
        raises ValueError."""
        out = []
        for r in self._visible_rows(min_pixels):
            k, n = int(r["label"]), int(r["n_pixels"])
            out.append({"label": k, "path": self._instance_paths[k] if self._instance_paths is not None else None, "pixels": n,
                        "bbox": (int(r["x_min"]), int(r["y_min"]), int(r["x_end"]) - 1, int(r["y_end"]) - 1),
                        "centre": (int(r["sum_x"]) / n, int(r["sum_y"]) / n), "nearest_m": float(r["z_min"])})
        return out

    def add_bounding_box_2d_tight_to_frame(self):
        """get_current_frame() also returns "bounding_box_2d_tight" from now on (needs collision_mesh=): {"data": a structured array
        with semanticId <u4 (= label + 1, the value instance_id_segmentation shows), x_min, y_min, x_max, y_max <i4 (inclusive) and
        occlusionRatio <f4 (always NaN: it is not computed), one record per visible label, "info": {"idToLabels": as
        instance_id_segmentation's}}.  It follows Isaac Sim's annotator of that name only as far as this shape: nothing of the
        reference depends on it, and the boxes are this project's own definition (tight around the pixels whose nearest collision-mesh
        hit has the label)."""
        if self._mesh is None:
            raise RuntimeError("instance ids come from the collision mesh: construct the camera with collision_mesh=")
        self._boxes_in_frame = True

    BOX_DTYPE = np.dtype([("semanticId", "<u4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"), ("y_max", "<i4"), ("occlusionRatio", "<f4")])

    def _bounding_boxes(self) -> dict:
        rows = self._visible_rows(1)
        data = np.zeros(len(rows), self.BOX_DTYPE)
        data["semanticId"] = rows["label"].astype(np.uint32) + 1
        data["x_min"], data["y_min"], data["x_max"], data["y_max"] = rows["x_min"], rows["y_min"], rows["x_end"] - 1, rows["y_end"] - 1
        data["occlusionRatio"] = np.nan
        return {"data": data, "info": {"idToLabels": self._id_to_labels(rows["label"])}}

    def get_instance_id_png(self) -> bytes:
        """The instance ids as a 16-bit grey PNG of id + 1 (0: nothing hit), encoded on the GPU by Renderer.encode_png's depth16 format
        with depth_scale 1 and depth_max 65535: integers below 2^24 are exact in fp32 and pass the encoder's truncation unchanged.
        More than 65 534 distinct labels do not fit and are refused."""
        ids = self._mesh_ids()
        n = len(self._instance_paths) if self._instance_paths is not None else int(ids.max().item()) + 1
        if n > 65534:
            raise ValueError(f"{n} labels do not fit a 16-bit PNG of id + 1 (at most 65534)")
        return self._r.encode_png((ids + 1).float().contiguous(), format="depth16", depth_scale=1.0, depth_max=65535.0)[0]

    # -- the exploration map: what the agent has SEEN, binned top-down on the GPU.  THIS PROJECT'S OWN observation (Renderer.topdown_map):
    # the reference's ExploredAreas / ExplorationCoverage count the 0.5 m cells the agent stood in (measures.py:399-437).
    def start_exploration_map(self, grid=None, model_to_map=None):
        """Starts (or restarts, empty) the map that update_exploration_map() accumulates: grid a TopdownGrid (default TopdownGrid()).
        The map is in WORLD coordinates — the coordinates of set_world_pose, where the scene stands after asset_model_to_world — with
        the stage's up axis Z as the height: cell (i, j) covers world x, y from the grid's origin.  model_to_map: a 3x4 from world
        coordinates to map coordinates (third coordinate the height) for a stage whose up axis is not Z, or a map frame of one's
        own; default the identity.  Needs collision_mesh=: the depth that is binned is the mesh's, the reference's source of depth."""
        import torch
        from .renderer import TopdownGrid
        if self._mesh is None:
            raise RuntimeError("the exploration map bins the collision mesh's depth: construct the camera with collision_mesh=")
        g = TopdownGrid() if grid is None else grid
        m = None if model_to_map is None else np.array(model_to_map, np.float64)
        cells = torch.zeros((int(g.ny), int(g.nx), 2), dtype=torch.int32, device=self._r.device)
        self._explore = (g, m, cells, torch.zeros((1, 4), dtype=torch.int32, device=self._r.device))

    def update_exploration_map(self):
        """Renders the collision mesh's depth at the current pose and adds it to the map, on the GPU; nothing crosses the link.
        Returns the frame's four counters as a device tensor (Renderer.topdown_map's counts[0])."""
        if self._explore is None:
            raise RuntimeError("start_exploration_map() first")
        g, m, cells, counts = self._explore
        cam = self._camera()
        self._r.topdown_map(self._mesh_depth(), self._r.pix_to_map(cam, m), g, out=(cells, counts), clear=False)
        return counts[0]

    def get_exploration_grid(self):
        """The map so far: int32 [ny, nx, 2] on the GPU (free hits, occupied hits per cell)."""
        if self._explore is None:
            raise RuntimeError("start_exploration_map() first")
        return self._explore[2]

    def get_exploration(self, min_hits: int = 1) -> dict:
        """Renderer.topdown_summary of the map so far: occupied_cells, free_cells, free_hits, occupied_hits, seen_cells, seen_area_m2."""
        return self._r.topdown_summary(self.get_exploration_grid(), min_hits, cell_size=self._explore[0].cell_size)

    def get_exploration_clearance(self, robot_radius_m: float = 0.1, min_hits: int = 1, unseen_blocks: bool = False):
        """Where the agent can stand, by what it has seen so far: a sage_gs.clearance.ClearanceMap of the exploration map (its
        occupied cells, with unseen_blocks also the cells not seen yet, grown by robot_radius_m), computed on the GPU.  Positions are
        the map's coordinates: world x, y unless start_exploration_map was given a model_to_map."""
        from .clearance import ClearanceMap
        cells = self.get_exploration_grid()
        return ClearanceMap.from_topdown(self._explore[0], cells, robot_radius_m, min_hits=min_hits, unseen_blocks=unseen_blocks, renderer=self._r)

    def get_depth(self, clip=(0.1, 6.5)) -> np.ndarray:
        """float32 [H,W] metres, limited to [0.1, 6.5] exactly as SimpleVLNEnv.get_depth does with the simulator's
        distance_to_image_plane (simple_env.py:1573-1578: astype(float32), np.clip(depth, 0.1, 6.5)); a pixel that hit
        nothing (inf) therefore reads 6.5.  With a collision mesh, from the mesh (the reference's source)."""
        depth = self._mesh_depth() if self._mesh is not None else self._rgb_depth()[1]
        if self._out is not None:        # the reference's order: clip (on the device, as the samples are loaded), then resize
            return self._resized(depth, "depth", None if clip is None else (float(clip[0]), float(clip[1]))).cpu().numpy()
        d = depth.cpu().numpy().astype(np.float32)
        return np.clip(d, clip[0], clip[1]) if clip is not None else d

    def add_distance_to_image_plane_to_frame(self):        # simple_env.py:850 — always available here
        return None


_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def _prim_body(text: str, header_re: str):
    """The `{ ... }` body of the first prim whose header matches, or None (brace matching; no nested parsing needed for
    the flat stanzas the reference's stages hold)."""
    m = re.search(header_re, text, re.S)
    if not m:
        return None
    i = text.find("{", m.end())
    if i < 0:
        return None
    depth, j = 0, i
    while j < len(text):
        if text[j] == "{":
            depth += 1
        elif text[j] == "}":
            depth -= 1
            if depth == 0:
                return text[i + 1:j]
        j += 1
    return None


def _vec3(body: str, name: str):
    m = re.search(r"\b(?:double3|float3|half3)\s+" + re.escape(name) + r"\s*=\s*\(\s*(" + _NUM + r")\s*,\s*(" + _NUM + r")\s*,\s*(" + _NUM + r")\s*\)", body)
    return tuple(float(m.group(k)) for k in (1, 2, 3)) if m else None


def parse_scene_usda(text: str) -> dict:
    """What a SAGE-3D scene stage (`{scene_id}.usda`, produced by `sage3d_usda_builder.build_usda_content` :93-149 from
    Data/template.usda) says about the Gaussian asset: the USDZ path referenced by /World/gauss
    (`prepend references = @...usdz[gauss.usda]@`, template.usda:115-117), the collision payload of
    /World/scene_collision (:156-158), and the gauss prim's transform ops — `double3 xformOp:rotateXYZ / :scale /
    :translate` and their `xformOpOrder` (:119-123) — plus the stage's upAxis and metersPerUnit (:105-108)."""
    out = {"usdz": None, "collision": None, "rotate_xyz": None, "scale": None, "translate": None, "xform_op_order": None,
           "up_axis": None, "meters_per_unit": None, "collision_ops": None}
    m = re.search(r"@([^@\n]+\.usdz)\[gauss\.usda\]@", text)
    if m:
        out["usdz"] = m.group(1)
    m = re.search(r"prepend\s+payload\s*=\s*@([^@\n]+)@", text)
    if m is None:
        m = re.search(r"@([^@\n]+_collision\.usd[ac]?)@", text)
    if m:
        out["collision"] = m.group(1)
    body = _prim_body(text, r'over\s+"gauss"\s*(?:\([^)]*\))?')
    if body is not None:
        out["rotate_xyz"] = _vec3(body, "xformOp:rotateXYZ")
        out["scale"] = _vec3(body, "xformOp:scale")
        out["translate"] = _vec3(body, "xformOp:translate")
        m = re.search(r"xformOpOrder\s*=\s*\[([^\]]*)\]", body)
        if m:
            out["xform_op_order"] = tuple(t.strip().strip('"') for t in m.group(1).split(",") if t.strip())
    body = _prim_body(text, r'(?:def|over)\s+(?:Xform\s+)?"scene_collision"\s*')
    if body is not None:
        from .mesh import split_prim
        out["collision_ops"] = split_prim(body, 0, len(body))[0]            # the prim's own attributes (its child prims cut out)
    m = re.search(r'upAxis\s*=\s*"([XYZ])"', text)
    if m:
        out["up_axis"] = m.group(1)
    m = re.search(r"metersPerUnit\s*=\s*(" + _NUM + ")", text)
    if m:
        out["meters_per_unit"] = float(m.group(1))
    return out


def collision_model_to_world(parsed: dict) -> np.ndarray:
    """The 4x4 model->world matrix of /World/scene_collision from `parse_scene_usda`'s `collision_ops` (its xformOps in
    `xformOpOrder`; identity when the stage has no such prim).  The template's (translate 0, orient (6.123234e-17, 0, 0, 1), scale 1)
    is a rotation by 180 degrees about Z (template.usda:156-165)."""
    from .mesh import xform_from_attrs
    ops = parsed.get("collision_ops")
    return xform_from_attrs(ops) if ops else np.eye(4)


def asset_model_to_world(parsed: dict) -> np.ndarray:
    """The 4x4 model->world matrix of the gauss prim from `parse_scene_usda`'s ops, applied in `xformOpOrder`
    (USD: the first op listed is the outermost; rotateXYZ = Rz Ry Rx for column vectors).  The template's
    (translate 0, rotateXYZ (-90,0,0), scale 1) gives `scenes.MODEL_TO_WORLD`.  The renderer takes rigid transforms
    only (the view must stay rigid): a scale other than 1 is refused here rather than silently mis-culled — rescale the
    Gaussians' means and scales instead."""
    import math
    order = parsed.get("xform_op_order") or ("xformOp:translate", "xformOp:rotateXYZ", "xformOp:scale")
    M = np.eye(4)
    for op in order:
        T = np.eye(4)
        if op == "xformOp:translate":
            T[:3, 3] = parsed.get("translate") or (0.0, 0.0, 0.0)
        elif op == "xformOp:rotateXYZ":
            rx, ry, rz = (math.radians(v) for v in (parsed.get("rotate_xyz") or (0.0, 0.0, 0.0)))
            cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
            Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
            T[:3, :3] = Rz @ Ry @ Rx
        elif op == "xformOp:scale":
            sc = parsed.get("scale") or (1.0, 1.0, 1.0)
            if any(abs(v - 1.0) > 1e-9 for v in sc):
                raise ValueError(f"xformOp:scale = {sc}: only rigid asset transforms are supported")
        else:
            raise ValueError(f"unsupported xform op {op!r}")
        M = M @ T
    return M
