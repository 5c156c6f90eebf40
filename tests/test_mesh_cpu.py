"""Mesh export without a GPU: the OBJ writer, Mesh extras and the outlier threshold rule, the configurations that are refused, the closed-form
Kuhn numbering against the explicit tables, the derived 16-case table, and the mesh entries of include/asd_hip.h at the C boundary (argument
checks answer before the HIP runtime is touched; the workspace size query is the sum of the layout the passes use)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from mesh_util import read_obj

P = C.c_void_p(0x1000)          # a non-NULL pointer that no accepted call may dereference on the host (and no launch happens in these tests)
NULL = C.c_void_p(0)
i32, i64 = C.c_int32, C.c_int64


def _lib():
    from scaledreamer_amd import _lib

    return _lib.lib()


# ---- Mesh, save_obj ---------------------------------------------------------------------------------------------------------------
def _tetrahedron():
    from scaledreamer_amd.mesh import Mesh

    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.2, 1.0 / 3.0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    return Mesh(v, f)


def test_save_obj_round_trip(tmp_path):
    from scaledreamer_amd.mesh import save_obj

    m = _tetrahedron()
    rgb = torch.tensor([[0.0, 0.25, 1.0], [0.1, 0.2, 0.3], [1.0, 1.0, 1.0], [1.0 / 3.0, 0.5, 0.75]])
    m.set_vertex_color(rgb)
    v, vn, f = read_obj(save_obj(str(tmp_path / "sub" / "a.obj"), m, save_normal=True, save_vertex_color=True))
    assert v.shape == (4, 6) and vn.shape == (4, 3) and f.shape == (4, 3, 3)
    np.testing.assert_array_equal(v[:, :3].astype(np.float32), m.v_pos.numpy())         # %.9g round-trips fp32
    np.testing.assert_array_equal(v[:, 3:].astype(np.float32), rgb.numpy())
    np.testing.assert_array_equal(vn.astype(np.float32), m.v_nrm.numpy())
    np.testing.assert_array_equal(f[:, :, 0], m.t_pos_idx.numpy() + 1)                   # 1-based, `a//a`
    np.testing.assert_array_equal(f[:, :, 2], m.t_pos_idx.numpy() + 1)
    assert (f[:, :, 1] == 0).all()
    lines = open(tmp_path / "sub" / "a.obj").read().splitlines()
    assert [l.split()[0] for l in lines] == ["v"] * 4 + ["vn"] * 4 + ["f"] * 4 and lines[8] == "f 1//1 3//3 2//2"
    v, vn, f = read_obj(save_obj(str(tmp_path / "b.obj"), m))
    assert v.shape == (4, 3) and vn.shape == (0,) and open(tmp_path / "b.obj").read().splitlines()[4] == "f 1// 3// 2//"
    with pytest.raises(ValueError):
        save_obj(str(tmp_path / "c.obj"), _tetrahedron(), save_vertex_color=True)


def test_mesh_extras_normals_and_threshold_rule():
    from scaledreamer_amd.mesh import Mesh, outlier_face_threshold

    m = Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long), grid_level=1, bbox="b")
    m.add_extra("more", 2)
    assert m.extras == {"grid_level": 1, "bbox": "b", "more": 2} and not m.requires_grad and m.v_rgb is None
    t = _tetrahedron()
    n = t.v_nrm
    assert n.shape == (4, 3) and torch.allclose(n.norm(dim=1), torch.ones(4), atol=1e-6)
    centre = t.v_pos.mean(0)
    assert ((t.v_pos - centre) * n).sum(-1).min() > 0, "outward-wound faces give outward vertex normals"
    assert Mesh(torch.zeros(2, 3), torch.zeros(0, 3, dtype=torch.long)).v_nrm.tolist() == [[0, 0, 1], [0, 0, 1]]
    # mesh.py:55-63: a float is a fraction of the largest component (int() truncates), an int is the face count
    assert outlier_face_threshold(1999, 0.01) == 19 and outlier_face_threshold(99, 0.01) == 0 and outlier_face_threshold(1000, 0.2) == 200
    assert outlier_face_threshold(1000, 50) == 50 and outlier_face_threshold(3, 1) == 1
    g = Mesh(torch.zeros(3, 3, requires_grad=True), torch.zeros(1, 3, dtype=torch.long))
    assert g.remove_outlier(0.5) is g, "a differentiable mesh is returned as it is"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_isosurface_methods_without_their_dependencies_name_mt_grid(tmp_path, monkeypatch):
    from scaledreamer_amd.geometry import BaseImplicitGeometry

    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="mt-grid"):
        BaseImplicitGeometry({"isosurface_method": "mc-cpu"}).isosurface()
    assert BaseImplicitGeometry.Config().isosurface_method == "mt"
    with pytest.raises(FileNotFoundError, match="mt-grid") as e:
        BaseImplicitGeometry({"isosurface_resolution": 64}).isosurface()
    assert "load/tets/64_tets.npz" in str(e.value)
    with pytest.raises(AttributeError):
        BaseImplicitGeometry({"isosurface_method": "dmtet"}).isosurface()
    with pytest.raises(NotImplementedError, match="not enabled"):
        BaseImplicitGeometry({"isosurface": False}).isosurface()


def test_exporter_refuses_the_uv_routes():
    from scaledreamer_amd import plugins  # noqa: F401
    from scaledreamer_amd.exporters import ExporterOutput, MeshExporter
    from scaledreamer_amd.registry import find

    assert find("mesh-exporter") is MeshExporter
    c = MeshExporter.Config()
    assert (c.fmt, c.save_name, c.save_normal, c.save_uv, c.save_texture, c.texture_size, c.texture_format, c.context_type, c.save_video) == \
        ("obj-mtl", "model", False, True, True, 1024, "jpg", "gl", False)
    kw = dict(geometry=None, material=None, background=None)
    for cfg in ({}, {"fmt": "obj-mtl", "save_uv": False}):
        with pytest.raises(NotImplementedError, match="xatlas.*nvdiffrast"):
            MeshExporter(cfg, **kw)
    with pytest.raises(NotImplementedError, match="xatlas.*nvdiffrast"):
        MeshExporter({"fmt": "obj"}, **kw)
    with pytest.raises(ValueError, match="fbx"):
        MeshExporter({"fmt": "fbx", "save_uv": False}, **kw)

    class Geo:
        def isosurface(self):
            return _tetrahedron()

        def export(self, points):
            return {"features": points}

    class Mat:
        def export(self, points, features):
            return {"albedo": features.clamp(0, 1)}

    (out,) = MeshExporter({"fmt": "obj", "save_uv": False, "save_name": "x", "save_normal": True}, geometry=Geo(), material=Mat(), background=None)()
    assert isinstance(out, ExporterOutput) and (out.save_name, out.save_type) == ("x.obj", "obj")
    assert out.params["save_vertex_color"] and out.params["save_normal"] and not out.params["save_mat"] and out.params["mesh"].v_rgb is not None
    (out,) = MeshExporter({"fmt": "obj", "save_uv": False, "save_texture": False}, geometry=Geo(), material=Mat(), background=None)()
    assert not out.params["save_vertex_color"] and out.params["mesh"].v_rgb is None


def test_no_material_export_is_the_clamped_albedo():
    from scaledreamer_amd.materials import NoMaterial

    f = torch.tensor([[-50.0, 0.0, 50.0]])
    out = NoMaterial({"n_output_dims": 3, "color_activation": "sigmoid"}).export(features=f, points=torch.zeros(1, 3))
    assert list(out) == ["albedo"] and torch.equal(out["albedo"], torch.sigmoid(f).clamp(0, 1))


# ---- the Kuhn numbering, the case table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 3, 6])
def test_kuhn_closed_form_numbering_is_the_explicit_tables(res):
    """vertex v owns edge slots 7 v + d - 1 (d = (di dj dk) of the far end) and cell c tet slots 6 c + t: the slots that stay inside the grid,
    in slot order, are the sorted unique edges of the explicit tables, and every tet edge of the explicit form is the slot the closed form
    gives (csrc/mesh.hip kuhn_edge_slot)"""
    from scaledreamer_amd.isosurface import BASE_TET_EDGES, KUHN_TETS, kuhn_grid_arrays

    verts, edges, tets, tet_edges = kuhn_grid_arrays(res)
    assert verts.shape == (res**3, 3) and tets.shape == (6 * (res - 1) ** 3, 4)
    assert (torch.linalg.det((verts[tets[:, 1:]] - verts[tets[:, :1]]).double()) > 0).all(), "all tets wound alike"
    slots, pairs = [], []
    for v in range(res**3):
        i, j, k = v // (res * res), (v // res) % res, v % res
        for d in range(1, 8):
            di, dj, dk = (d >> 2) & 1, (d >> 1) & 1, d & 1
            if i + di < res and j + dj < res and k + dk < res:
                slots.append(7 * v + d - 1)
                pairs.append((v, v + di * res * res + dj * res + dk))
    assert edges.tolist() == [list(p) for p in pairs], "slot order is the order of the reference's sorted unique edges"
    rank = {s: n for n, s in enumerate(slots)}
    voff = lambda code: ((code >> 2) & 1) * res * res + ((code >> 1) & 1) * res + (code & 1)
    want = []
    for i, j, k in itertools.product(range(res - 1), repeat=3):
        vc = (i * res + j) * res + k
        for o in KUHN_TETS:
            want.append([rank[7 * (vc + voff(min(o[a], o[b]))) + (o[a] ^ o[b]) - 1] for a, b in zip(BASE_TET_EDGES[0::2], BASE_TET_EDGES[1::2])])
    assert tet_edges.tolist() == want
    if res == 6:
        assert (verts.shape[0], tets.shape[0]) == (216, 750)


def test_case_table_follows_its_derivation():
    """asd_mt_case_table is the table the kernels read.  On the tet (0, e_x, e_y, e_z) (det > 0) with crossings at the edge mid-points every
    triangle's normal points to the positive side, the triangles of a case tile its crossing edges, and complementary cases are mirror images."""
    buf = (C.c_int32 * 112)()
    assert _lib().asd_mt_case_table(buf) == 0
    tab = np.asarray(list(buf)).reshape(16, 7)
    assert tab[:, 0].tolist() == [bin(c).count("1") % 4 and (2 if bin(c).count("1") == 2 else 1) for c in range(16)]
    corner = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    ends = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for c in range(16):
        n = tab[c, 0]
        ids = tab[c, 1:1 + 3 * n]
        assert (tab[c, 1 + 3 * n:] == -1).all()
        pos = [v for v in range(4) if (c >> v) & 1]
        crossing = {e for e, (a, b) in enumerate(ends) if ((c >> a) & 1) != ((c >> b) & 1)}
        assert set(ids.tolist()) == crossing
        if n == 0:
            continue
        toward = corner[pos].mean(0) - corner[[v for v in range(4) if v not in pos]].mean(0)
        mid = np.asarray([(corner[a] + corner[b]) / 2 for a, b in ends])
        for tri in ids.reshape(n, 3):
            assert len(set(tri.tolist())) == 3
            assert np.dot(np.cross(mid[tri[1]] - mid[tri[0]], mid[tri[2]] - mid[tri[0]]), toward) > 0, (c, tri)
        if n == 2:      # the two triangles share exactly the diagonal, run through it in opposite directions
            a, b = ids.reshape(2, 3).tolist()
            da = {(a[q], a[(q + 1) % 3]) for q in range(3)}
            db = {(b[(q + 1) % 3], b[q]) for q in range(3)}
            assert len(da & db) == 1
            assert set(next(iter(da & db))) in ({1, 4}, {2, 3}), "the diagonal joins 02|13, else 03|12"


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def _rejected(name, args, word=None):
    lib = _lib()
    rc = getattr(lib, name)(*args)
    err = lib.asd_last_error()
    return rc == 1 and name.encode() in err and (word is None or word.encode() in err)      # ASD_ERR_ARG


def test_entries_are_declared_listed_and_exported():
    import os
    import re

    from scaledreamer_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asd_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(asd_[a-z0-9_]+)\s*\(", src))
    for n in ["asd_mt_workspace", "asd_mt_count", "asd_mt_emit", "asd_mt_case_table", "asd_scan_i32_blocks_workspace", "asd_scan_i32_blocks",
              "asd_mesh_cc_round", "asd_mesh_face_counts", "asd_mesh_keep", "asd_mesh_compact"]:
        assert n in declared and n in _lib.SYMBOLS and hasattr(_lib.lib(), n), n


def test_null_and_negative_arguments_are_reported():
    z, n = i64(0), i64(5)
    assert _rejected("asd_mt_case_table", [NULL])
    assert _rejected("asd_mt_workspace", [i32(8), z, z, NULL, NULL])
    out = i64(0)
    for res in (1, -3, 513):
        assert _rejected("asd_mt_workspace", [i32(res), z, z, NULL, C.byref(out)], "res")
    assert _rejected("asd_mt_workspace", [i32(0), i64(-1), z, NULL, C.byref(out)]) and _rejected("asd_mt_workspace", [i32(0), z, i64(-1), NULL, C.byref(out)])
    assert _rejected("asd_scan_i32_blocks_workspace", [n, NULL]) and _rejected("asd_scan_i32_blocks_workspace", [i64(-1), C.byref(out)])
    assert _rejected("asd_scan_i32_blocks_workspace", [i64(2**31), C.byref(out)])
    ok = [P, n, P, P, P, NULL]
    for idx in (0, 2, 3, 4):
        bad = list(ok)
        bad[idx] = NULL
        assert _rejected("asd_scan_i32_blocks", bad), idx
    assert _rejected("asd_scan_i32_blocks", [P, i64(-1), P, P, P, NULL]) and _rejected("asd_scan_i32_blocks", [C.c_void_p(0x1004), n, P, P, P, NULL], "aligned")
    # asd_mt_count(level, res, n_grid, edges, n_edges, tet_verts, n_tets, workspace, stream)
    assert _rejected("asd_mt_count", [NULL, i32(8), z, NULL, z, NULL, z, P, NULL]) and _rejected("asd_mt_count", [P, i32(8), z, NULL, z, NULL, z, NULL, NULL])
    assert _rejected("asd_mt_count", [P, i32(1), z, NULL, z, NULL, z, P, NULL], "res") and _rejected("asd_mt_count", [P, i32(0), n, NULL, n, P, n, P, NULL], "tables")
    assert _rejected("asd_mt_count", [P, i32(0), n, P, n, NULL, n, P, NULL], "tables") and _rejected("asd_mt_count", [P, i32(0), i64(-1), P, n, P, n, P, NULL])
    assert _rejected("asd_mt_count", [P, i32(0), n, P, i64(-2), P, n, P, NULL]) and _rejected("asd_mt_count", [P, i32(8), z, NULL, z, NULL, z, C.c_void_p(0x1004), NULL], "aligned")
    # asd_mt_emit(level, res, axis, verts, n_grid, edges, n_edges, tet_verts, tet_edges, n_tets, workspace, n_verts_out, n_faces_out, out_verts, out_faces, stream)
    kuhn = [P, i32(8), P, NULL, z, NULL, z, NULL, NULL, z, P, n, n, P, P, NULL]
    for idx, word in ((0, None), (2, "axis"), (10, None), (13, "output"), (14, "output")):
        bad = list(kuhn)
        bad[idx] = NULL
        assert _rejected("asd_mt_emit", bad, word), idx
    for idx in (11, 12):
        bad = list(kuhn)
        bad[idx] = i64(-1)
        assert _rejected("asd_mt_emit", bad, "negative"), idx
    explicit = [P, i32(0), NULL, P, n, P, n, P, P, n, P, n, n, P, P, NULL]
    for idx in (3, 5, 7, 8):
        bad = list(explicit)
        bad[idx] = NULL
        assert _rejected("asd_mt_emit", bad, "tables"), idx
    # asd_mesh_cc_round(faces, n_faces, n_verts, first, labels, changed, stream)
    assert _rejected("asd_mesh_cc_round", [NULL, n, n, i32(1), P, P, NULL]) and _rejected("asd_mesh_cc_round", [P, n, n, i32(1), NULL, P, NULL])
    assert _rejected("asd_mesh_cc_round", [P, n, n, i32(1), P, NULL, NULL]) and _rejected("asd_mesh_cc_round", [P, i64(-1), n, i32(1), P, P, NULL])
    assert _rejected("asd_mesh_cc_round", [P, n, i64(-1), i32(1), P, P, NULL])
    # asd_mesh_face_counts(faces, n_faces, n_verts, labels, counts, stream)
    for idx in (0, 3, 4):
        bad = [P, n, n, P, P, NULL]
        bad[idx] = NULL
        assert _rejected("asd_mesh_face_counts", bad), idx
    assert _rejected("asd_mesh_face_counts", [P, i64(-1), n, P, P, NULL]) and _rejected("asd_mesh_face_counts", [P, n, i64(-1), P, P, NULL])
    # asd_mesh_keep(faces, n_faces, n_verts, labels, counts, threshold, v_keep, f_keep, stream)
    for idx in (0, 3, 4, 6, 7):
        bad = [P, n, n, P, P, i32(1), P, P, NULL]
        bad[idx] = NULL
        assert _rejected("asd_mesh_keep", bad), idx
    assert _rejected("asd_mesh_keep", [P, i64(-1), n, P, P, i32(1), P, P, NULL])
    # asd_mesh_compact(v_pos, faces, n_verts, n_faces, v_keep, v_map, f_keep, f_map, n_verts_out, n_faces_out, v_out, f_out, stream)
    okc = [P, P, n, n, P, P, P, P, n, n, P, P, NULL]
    for idx in (0, 1, 4, 5, 6, 7, 10, 11):
        bad = list(okc)
        bad[idx] = NULL
        assert _rejected("asd_mesh_compact", bad), idx
    for idx, val in ((2, -1), (3, -1), (8, -1), (9, -1), (8, 6), (9, 6)):
        bad = list(okc)
        bad[idx] = i64(val)
        assert _rejected("asd_mesh_compact", bad), (idx, val)


def test_empty_inputs_are_ok_without_a_launch():
    lib = _lib()
    assert lib.asd_mesh_face_counts(NULL, i64(0), i64(0), NULL, NULL, NULL) == 0
    assert lib.asd_mesh_keep(NULL, i64(0), i64(0), NULL, NULL, i32(1), NULL, NULL, NULL) == 0
    assert lib.asd_mesh_compact(NULL, NULL, i64(0), i64(0), NULL, NULL, NULL, NULL, i64(0), i64(0), NULL, NULL, NULL) == 0


@pytest.mark.parametrize("res,n_edges,n_tets", [(6, 0, 0), (9, 0, 0), (128, 0, 0), (0, 1115, 750), (0, 1, 1), (0, 0, 0), (0, 9_500_000, 1_572_864)])
def test_workspace_query_is_the_sum_of_the_layout(res, n_edges, n_tets):
    """asd_mt_workspace's total, the layout it reports (the one asd_mt_count / asd_mt_emit carve the workspace with) and the scan's own size
    query agree: regions in declaration order, each rounded up to 64 int32 (256 bytes), nothing else"""
    from scaledreamer_amd._lib import MtLayout

    lib = _lib()
    lay, total, scan = MtLayout(), i64(-1), i64(-1)
    assert lib.asd_mt_workspace(i32(res), i64(n_edges), i64(n_tets), C.byref(lay), C.byref(total)) == 0
    E = 7 * res**3 if res else n_edges
    T = 6 * (res - 1) ** 3 if res else n_tets
    assert (lay.n_edge_slots, lay.n_tet_slots) == (E, T)
    assert lib.asd_scan_i32_blocks_workspace(i64(max(E, T)), C.byref(scan)) == 0 and scan.value == -(-max(E, T) // 2048)
    up = lambda n: (n + 63) // 64 * 64
    sizes = [E, T, scan.value, 2]
    offsets = [lay.edge_off, lay.tet_off, lay.scan, lay.counts]
    assert offsets == [sum(up(s) for s in sizes[:q]) for q in range(4)]
    assert total.value == lay.total == sum(up(s) for s in sizes)
    only = i64(-1)
    assert lib.asd_mt_workspace(i32(res), i64(n_edges), i64(n_tets), NULL, C.byref(only)) == 0 and only.value == total.value
