"""Triangle meshes from ASCII USD (`.usda`) — the collision payload of a SAGE-3D scene (`{scene_id}_collision.usd`, placed by the
template's /World/scene_collision prim, Data/template.usda:156-165), which the reference renders for its depth channel
(simple_env.py:1395-1589).  No `pxr` is needed: `read_usda_mesh` reads every `def Mesh` of an ASCII layer — `point3f[] points`,
`int[] faceVertexCounts`, `int[] faceVertexIndices` — fan-triangulates its polygons and applies the transform ops of the prim and of
every prim enclosing it (`xformOp:translate / orient / rotateXYZ / rotateX|Y|Z / scale / transform`, in `xformOpOrder`) and the layer's
`metersPerUnit`.  Binary crate files (`PXR-USDC`) are refused: convert them with `usdcat in.usd -o out.usda` where USD is installed.
References, payloads, variants and time samples inside the mesh layer are not followed.  NumPy only (no torch).
"""
from __future__ import annotations

import math
import re
from typing import Tuple

import numpy as np

_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[-+]?inf|nan"
_PRIM = re.compile(r'\b(def|over|class)\s+(?:([A-Za-z_][\w:]*)\s+)?"([^"]*)"\s*')


def _nums(s: str) -> np.ndarray:
    return np.array([float(x) for x in re.findall(_NUM, s)], np.float64)


def _match(text: str, i: int, open_c: str, close_c: str) -> int:
    """Index of the bracket closing the one at text[i] (strings skipped)."""
    depth, j, n = 0, i, len(text)
    while j < n:
        c = text[j]
        if c == '"':
            j = text.index('"', j + 1)
        elif c == open_c:
            depth += 1
        elif c == close_c:
            depth -= 1
            if depth == 0:
                return j
        j += 1
    raise ValueError(f"unbalanced {open_c}{close_c} in USDA text")


def _strip_comments(text: str) -> str:
    out = []
    for line in text.splitlines():
        q, cut = False, None
        for k, c in enumerate(line):
            if c == '"':
                q = not q
            elif c == "#" and not q:
                cut = k
                break
        out.append(line if cut is None else line[:cut])
    return "\n".join(out)


def _rot(axis: str, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return {"X": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "Y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "Z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def quat_wxyz_to_matrix(q) -> np.ndarray:
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def xform_from_attrs(body: str) -> np.ndarray:
    """The 4x4 local transform (column vectors) a prim's own attributes define: its `xformOpOrder`, first op outermost (USD's
    convention, as adapter.asset_model_to_world); identity without one.  `body` is the prim's text WITHOUT its child prims."""
    m = re.search(r"xformOpOrder\s*=\s*\[([^\]]*)\]", body)
    M = np.eye(4)
    if not m:
        return M
    for tok in (t.strip().strip('"') for t in m.group(1).split(",") if t.strip()):
        inv = tok.startswith("!invert!")
        name = tok[len("!invert!"):] if inv else tok
        v = re.search(r"(?:^|[\s(])(?:[\w\[\]]+\s+)?" + re.escape(name) + r"\s*=\s*", body)
        if not v:
            raise ValueError(f"xformOpOrder names {name!r}, which the prim does not define")
        kind = name.split(":")[1] if ":" in name else name
        j = v.end()
        T = np.eye(4)
        if kind == "transform":
            k = _match(body, j, "(", ")")
            T = _nums(body[j:k + 1]).reshape(4, 4).T                     # USD matrices act on row vectors
        elif kind.startswith("rotate") and len(kind) == 7:                # rotateX / rotateY / rotateZ: one angle in degrees
            T[:3, :3] = _rot(kind[6], float(re.match(r"\s*(" + _NUM + ")", body[j:]).group(1)))
        else:
            k = _match(body, j, "(", ")")
            val = _nums(body[j:k + 1])
            if kind == "translate":
                T[:3, 3] = val
            elif kind == "scale":
                T[:3, :3] = np.diag(val)
            elif kind == "orient":
                T[:3, :3] = quat_wxyz_to_matrix(val)
            elif kind.startswith("rotate") and len(kind) == 9:          # rotateXYZ etc.: the first axis listed is applied first
                R = np.eye(3)
                for ax, deg in zip(kind[6:], val):
                    R = _rot(ax, deg) @ R
                T[:3, :3] = R
            else:
                raise ValueError(f"unsupported xform op {name!r}")
        M = M @ (np.linalg.inv(T) if inv else T)
    return M


def split_prim(text: str, start: int, end: int):
    """(own text, [(type, name, body_start, body_end)]) of the block text[start:end]: the child prims' bodies cut out of it."""
    own, kids, pos = [], [], start
    while True:
        m = _PRIM.search(text, pos, end)
        if not m:
            own.append(text[pos:end])
            return "".join(own), kids
        own.append(text[pos:m.start()])
        j = m.end()
        if j < end and text[j] == "(":
            j = _match(text, j, "(", ")") + 1
        b = text.find("{", j, end)
        if b < 0:
            raise ValueError(f"prim {m.group(3)!r} has no body")
        e = _match(text, b, "{", "}")
        kids.append((m.group(2), m.group(3), b + 1, e))
        pos = e + 1


def _array(own: str, name: str):
    m = re.search(r"\b" + re.escape(name) + r"\s*=\s*\[", own)
    if not m:
        return None
    k = _match(own, m.end() - 1, "[", "]")
    return _nums(own[m.end():k])


def fan_triangulate(counts: np.ndarray, indices: np.ndarray) -> np.ndarray:
    """[F,3] triangles of polygons given as USD faceVertexCounts / faceVertexIndices: polygon (i0, i1, ..., ik) -> (i0, ij, ij+1)."""
    counts = np.asarray(counts, np.int64)
    indices = np.asarray(indices, np.int64)
    if counts.sum() != len(indices):
        raise ValueError(f"faceVertexCounts sum to {int(counts.sum())}, faceVertexIndices has {len(indices)} entries")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    nt = np.maximum(counts - 2, 0)
    face = np.repeat(np.arange(len(counts)), nt)
    k = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    s = starts[face]
    return np.stack([indices[s], indices[s + k + 1], indices[s + k + 2]], 1) if len(face) else np.zeros((0, 3), np.int64)


def parse_usda_mesh_text(text: str, return_prims: bool = False):
    """read_usda_mesh of a layer given as text."""
    text = _strip_comments(text)
    mpu = 1.0
    head = re.match(r"\s*\(", text)
    root_start = 0
    if head:
        k = _match(text, head.end() - 1, "(", ")")
        m = re.search(r"metersPerUnit\s*=\s*(" + _NUM + ")", text[:k])
        if m:
            mpu = float(m.group(1))
        root_start = k + 1
    verts, tris, n_off = [], [], 0
    tri_prim, prim_paths = [], []

    def walk(start, end, parent, kind, path=""):
        nonlocal n_off
        own, kids = split_prim(text, start, end)
        M = parent @ xform_from_attrs(own) if kind is not None else parent
        if kind == "Mesh":
            pts, cnt, idx = _array(own, "points"), _array(own, "faceVertexCounts"), _array(own, "faceVertexIndices")
            if pts is not None and cnt is not None and idx is not None and len(pts):
                p = pts.reshape(-1, 3)
                t = fan_triangulate(cnt.astype(np.int64), idx.astype(np.int64))
                if len(t) and (t.min() < 0 or t.max() >= len(p)):
                    raise ValueError("faceVertexIndices outside the mesh's points")
                verts.append(p @ M[:3, :3].T + M[:3, 3])
                tris.append(t + n_off)
                n_off += len(p)
                if len(t):                                              # a Mesh that contributes triangles: the next index
                    tri_prim.append(np.full(len(t), len(prim_paths), np.int32))
                    prim_paths.append(path)
        for ktype, name, b, e in kids:
            walk(b, e, M, ktype or "", path + "/" + name)

    S = np.eye(4)
    S[:3, :3] *= mpu
    walk(root_start, len(text), S, None)
    V, T = (np.concatenate(verts), np.concatenate(tris)) if verts else (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64))
    if not return_prims:
        return V, T
    return V, T, (np.concatenate(tri_prim) if tri_prim else np.zeros(0, np.int32)), prim_paths


def read_usda_mesh(path: str, return_prims: bool = False):
    """(vertices float64 [V,3] in metres, triangles int64 [F,3]) of every `def Mesh` in the ASCII USD layer at `path`, in the layer's
    root frame (each mesh's own and enclosing transform ops and the layer's metersPerUnit applied).
    return_prims=True: (vertices, triangles, tri_prim, prim_paths) — which Mesh prim each triangle came from: tri_prim int32 [F] indexes
    prim_paths, the full prim paths (such as /World/scene_collision/chair_3/mesh) of the Mesh prims that contribute triangles, numbered
    in traversal order (depth first, children in file order).  These are the labels of Renderer.render_mesh_ids."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] == b"PXR-USDC":
        raise ValueError(f"{path} is a binary USD crate file, which sage_gs does not parse: convert it to ASCII first "
                         f"(`usdcat {path} -o {path.rsplit('.', 1)[0]}.usda` where USD is installed) and pass the .usda")
    return parse_usda_mesh_text(data.decode("utf-8", "replace"), return_prims)
