"""Which `def Mesh` prim a triangle came from (mesh.read_usda_mesh(return_prims=True)) and which object of the synthetic room
(scenes.make_room_mesh_parts): the labels of the object-id channel.  CPU only, no native code."""
import numpy as np

from sage_gs import mesh as mesh_io
from sage_gs import scenes

USDA = '''#usda 1.0
(
    defaultPrim = "World"
    metersPerUnit = 1
    upAxis = "Z"
)

def Xform "World"
{
    def Xform "scene_collision"
    {
        def Xform "chair_3"
        {
            double3 xformOp:translate = (1, 0, 0)
            uniform token[] xformOpOrder = ["xformOp:translate"]

            def Mesh "mesh"
            {
                int[] faceVertexCounts = [4]
                int[] faceVertexIndices = [0, 1, 2, 3]
                point3f[] points = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
            }
        }
        def Mesh "no_points"
        {
            int[] faceVertexCounts = [3]
            int[] faceVertexIndices = [0, 1, 2]
        }
        def Xform "table"
        {
            def Mesh "no_faces"
            {
                int[] faceVertexCounts = []
                int[] faceVertexIndices = []
                point3f[] points = [(0, 0, 0), (1, 0, 0), (1, 1, 0)]
            }
            def Xform "top"
            {
                def Mesh "mesh"
                {
                    int[] faceVertexCounts = [3, 3, 3]
                    int[] faceVertexIndices = [0, 1, 2, 0, 2, 3, 0, 3, 1]
                    point3f[] points = [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 2)]
                }
            }
        }
    }
    def Mesh "floor"
    {
        int[] faceVertexCounts = [3]
        int[] faceVertexIndices = [0, 1, 2]
        point3f[] points = [(0, 0, 0), (5, 0, 0), (0, 5, 0)]
    }
}
'''


def test_prims_of_nested_meshes_in_traversal_order(tmp_path):
    V, T, tri_prim, paths = mesh_io.parse_usda_mesh_text(USDA, return_prims=True)
    # a Mesh without points and one without faces contribute no triangle and get no index; the others are numbered depth first
    assert paths == ["/World/scene_collision/chair_3/mesh", "/World/scene_collision/table/top/mesh", "/World/floor"]
    assert tri_prim.dtype == np.int32 and tri_prim.tolist() == [0, 0, 1, 1, 1, 2]
    assert len(T) == len(tri_prim) == 6
    # the triangles of prim k index that prim's own vertices (the no_faces Mesh's three points sit between chair and table top)
    assert T[tri_prim == 0].max() <= 3 and T[tri_prim == 1].min() >= 7 and T[tri_prim == 2].min() >= 11
    assert np.allclose(V[0], [1, 0, 0])                                           # chair_3's translate applied
    p = tmp_path / "c.usda"
    p.write_text(USDA)
    V2, T2, tp2, paths2 = mesh_io.read_usda_mesh(str(p), return_prims=True)
    assert np.array_equal(V2, V) and np.array_equal(T2, T) and np.array_equal(tp2, tri_prim) and paths2 == paths


def test_return_prims_false_is_unchanged(tmp_path):
    plain = mesh_io.parse_usda_mesh_text(USDA)
    assert isinstance(plain, tuple) and len(plain) == 2
    V, T, _, _ = mesh_io.parse_usda_mesh_text(USDA, return_prims=True)
    assert np.array_equal(plain[0], V) and np.array_equal(plain[1], T) and plain[1].dtype == np.int64 and plain[0].dtype == np.float64
    p = tmp_path / "c.usda"
    p.write_text(USDA)
    again = mesh_io.read_usda_mesh(str(p))
    assert len(again) == 2 and np.array_equal(again[0], V) and np.array_equal(again[1], T)
    empty = mesh_io.parse_usda_mesh_text('#usda 1.0\n\ndef Xform "W"\n{\n}\n', return_prims=True)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,) and empty[2].dtype == np.int32 and empty[3] == []


def test_make_room_mesh_parts_equals_make_room_mesh():
    for n, seed in ((2000, 1), (20000, 1), (3000, 7)):
        m = scenes.make_room_mesh(n, seed=seed)
        V, T, part = scenes.make_room_mesh_parts(n, seed=seed)
        assert np.array_equal(V, m.vertices) and np.array_equal(T, m.triangles)
        assert part.dtype == np.int32 and part.shape == (len(T),) and sorted(np.unique(part).tolist()) == list(range(12))
        assert len(scenes.ROOM_MESH_PARTS) == 12
        assert (np.diff(part) >= 0).all()                                       # the parts follow one another, as make_room_mesh lists them
        # no vertex is shared between two parts, and each part is a closed surface (every edge in exactly two triangles)
        owner = np.full(len(V), -1)
        for k in range(12):
            t = T[part == k]
            assert (owner[t.reshape(-1)] == -1).all(), (n, seed, k)
            owner[t.reshape(-1)] = k
            e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
            _, cnt = np.unique(e, axis=0, return_counts=True)
            assert (cnt == 2).all(), (n, seed, k)
        # the shell is the gridded room box (part 0), the spheres are icospheres (20 * 4^level triangles), the cylinders are equal
        c = np.bincount(part)
        assert c[7] == c[8] and c[7] % 20 == 0 and c[9] == c[10] == c[11] and c[0] == c.max()
