"""The per-face UV atlas without a GPU: asd_atlas_layout (a host function) against its plain-Python restatement, the exporter's new
configuration keys, and the OBJ / MTL / texture writer on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from atlas_util import MAX_T, layout_ref, read_obj_uv, smallest_texture_size


def _layout(F, T, g):
    """-> ((n, c, L), None) or (None, the error message)"""
    from scaledreamer_amd import _lib

    lay = _lib.AtlasLayout()
    rc = _lib.lib().asd_atlas_layout(C.c_int64(F), C.c_int32(T), C.c_int32(g), C.byref(lay))
    if rc != 0:
        return None, _lib.lib().asd_last_error().decode()
    assert (lay.n_faces, lay.texture_size, lay.gutter) == (F, T, g)
    return (lay.n, lay.c, lay.L), None


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("T", [7, 16, 50, 1024, 8192])
def test_layout_equals_its_restatement(T, g):
    for F in (0, 1, 2, 3, 5, 8, 9, 131072, 131073):
        want = layout_ref(F, T, g)
        got, err = _layout(F, T, g)
        assert got == want, (F, T, g, got, want, err)
        if want is not None:
            n, c, L = want
            assert F == 0 or (L >= 1 and n * c <= T and 2 * n * n >= F and c - g >= g + L + 1), (F, T, g, want)
            continue
        # refused exactly when L < 1; the message names F, T, g and the smallest texture_size that fits
        assert "asd_atlas_layout" in err and f"{F} faces" in err and f"texture_size of {T} " in err and f"gutter {g} " in err, err
        fit = int(re.search(r"smallest texture_size that fits is (\d+)", err).group(1))
        assert fit == smallest_texture_size(F, g) > T
        if fit <= MAX_T:
            assert "beyond the limit" not in err
            assert _layout(F, fit, g)[0] == layout_ref(F, fit, g) and layout_ref(F, fit, g) is not None
            assert _layout(F, fit - 1, g)[0] is None and layout_ref(F, fit - 1, g) is None
        else:
            assert "beyond the limit of 8192" in err


def test_layout_argument_checks_and_capacity():
    from scaledreamer_amd import _lib, ops

    for F, T, g, word in ((-1, 16, 1, "n_faces"), (2**31, 16, 1, "n_faces"), (4, 0, 1, "texture_size"), (4, 8193, 1, "texture_size"), (4, 16, -1, "gutter")):
        got, err = _layout(F, T, g)
        assert got is None and word in err, (F, T, g, err)
    assert _lib.lib().asd_atlas_layout(C.c_int64(4), C.c_int32(16), C.c_int32(1), None) == 1
    # the default texture (1024, gutter 1): cells of side 5 are the smallest with a leg, 204 per row, two faces each
    assert _layout(2 * 204 * 204, 1024, 1)[0] == (204, 5, 1) and _layout(2 * 204 * 204 + 1, 1024, 1)[0] is None
    lay = ops.atlas_layout(9, 50, 2)        # the Python entry reads the same struct
    assert (lay.n_faces, lay.texture_size, lay.gutter, lay.n, lay.c, lay.L) == (9, 50, 2, 3, 16, 9)
    with pytest.raises(_lib.AsdError, match="smallest texture_size that fits is 24"):
        ops.atlas_layout(9, 16, 2)


def test_entries_are_declared_listed_and_exported_and_check_their_arguments():
    from scaledreamer_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asd_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(asd_[a-z0-9_]+)\s*\(", src))
    for name in ("asd_atlas_layout", "asd_atlas_uv", "asd_atlas_bake", "asd_atlas_pack_u8"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    lib = _lib.lib()
    P, NULL, i64, i32 = C.c_void_p(0x1000), C.c_void_p(0), C.c_int64, C.c_int32       # P: never dereferenced by a refused call, and nothing launches here
    lay = _lib.AtlasLayout()
    assert lib.asd_atlas_layout(i64(4), i32(16), i32(1), C.byref(lay)) == 0
    rejected = lambda rc, word: rc == 1 and word.encode() in lib.asd_last_error()
    assert rejected(lib.asd_atlas_uv(None, i64(4), P, P, NULL), "null")
    assert rejected(lib.asd_atlas_uv(C.byref(lay), i64(5), P, P, NULL), "layout") and rejected(lib.asd_atlas_uv(C.byref(lay), i64(4), NULL, P, NULL), "null")
    assert rejected(lib.asd_atlas_bake(C.byref(lay), P, P, i64(4), i64(3), P, P, P, NULL), "layout")
    assert rejected(lib.asd_atlas_bake(C.byref(lay), P, P, i64(4), i64(4), NULL, P, P, NULL), "null")
    assert rejected(lib.asd_atlas_bake(C.byref(lay), NULL, P, i64(4), i64(4), P, P, P, NULL), "null")
    assert rejected(lib.asd_atlas_bake(C.byref(lay), P, P, i64(-1), i64(4), P, P, P, NULL), "n_verts")
    assert rejected(lib.asd_atlas_bake(C.byref(lay), P, P, i64(4), i64(4), C.c_void_p(0x1004), P, P, NULL), "aligned")
    forged = _lib.AtlasLayout(4, 16, 1, 1, 16, 14)      # a leg that would reach into the other face's half
    assert rejected(lib.asd_atlas_bake(C.byref(forged), P, P, i64(4), i64(4), P, P, P, NULL), "layout")
    assert rejected(lib.asd_atlas_pack_u8(P, P, i64(5), i32(5), P, i64(16), NULL), "C must")
    assert rejected(lib.asd_atlas_pack_u8(P, P, i64(-1), i32(3), P, i64(16), NULL), "n_owned")
    assert rejected(lib.asd_atlas_pack_u8(NULL, P, i64(5), i32(3), P, i64(16), NULL), "null")
    assert lib.asd_atlas_pack_u8(NULL, NULL, i64(0), i32(3), NULL, i64(16), NULL) == 0      # nothing to pack: no launch
    empty = _lib.AtlasLayout()
    assert lib.asd_atlas_layout(i64(0), i32(16), i32(1), C.byref(empty)) == 0 and lib.asd_atlas_uv(C.byref(empty), i64(0), NULL, NULL, NULL) == 0


# ---- the exporter's configuration -----------------------------------------------------------------------------------------------------
def test_exporter_configuration():
    from scaledreamer_amd import plugins  # noqa: F401
    from scaledreamer_amd.exporters import MeshExporter

    c = MeshExporter.Config()
    assert (c.uv_method, c.uv_gutter, c.texture_chunk) == ("xatlas", 1, 1 << 20)
    kw = dict(geometry=None, material=None, background=None)
    with pytest.raises(NotImplementedError, match="xatlas.*nvdiffrast.*face-cells"):     # the refusal names the alternative
        MeshExporter({}, **kw)
    for cfg in ({"uv_method": "face-cells"}, {"uv_method": "face-cells", "fmt": "obj-mtl"}, {"uv_method": "face-cells", "fmt": "obj", "save_uv": True},
                {"uv_method": "face-cells", "fmt": "obj", "save_uv": False}, {"uv_method": "face-cells", "fmt": "obj-mtl", "save_uv": False, "save_texture": False}):
        MeshExporter(cfg, **kw)
    with pytest.raises(ValueError, match="charts"):
        MeshExporter({"uv_method": "charts", "fmt": "obj", "save_uv": False}, **kw)
    with pytest.raises(ValueError, match="save_uv must be True when save_texture is True"):
        MeshExporter({"uv_method": "face-cells", "fmt": "obj-mtl", "save_uv": False}, **kw)
    with pytest.raises(ValueError, match="fbx"):
        MeshExporter({"uv_method": "face-cells", "fmt": "fbx"}, **kw)


def test_mesh_uv_attributes():
    from scaledreamer_amd._lib import AsdError
    from scaledreamer_amd.mesh import Mesh

    m = Mesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]))
    with pytest.raises(ValueError, match="xatlas"):
        m.unwrap_uv("xatlas")
    with pytest.raises(AsdError, match="no CPU fallback"):
        m.v_tex      # unwraps on first use, as the reference's property does, and that runs on the device only
    vt, ft = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), torch.tensor([[0, 1, 2]])
    m.set_uv(vt, ft)
    assert m.v_tex is vt and m.t_tex_idx is ft and m.atlas is None


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
def _textured_tetrahedron():
    from scaledreamer_amd.mesh import Mesh

    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.2, 1.0 / 3.0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    m = Mesh(v, f)
    vt = torch.tensor([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [1.0, 1.0], [0.5, 1.0], [1.0, 0.5], [0.25, 0.125], [0.75, 0.0], [0.0, 0.3], [1.0, 0.0], [0.0, 1.0],
                       [0.625, 0.375]])
    m.set_uv(vt, torch.arange(12).view(4, 3).flip(0))
    return m


def test_save_obj_with_material_and_texture(tmp_path):
    from PIL import Image

    from scaledreamer_amd.mesh import save_obj

    m = _textured_tetrahedron()
    kd = torch.arange(48, dtype=torch.uint8).view(4, 4, 3) * 5
    paths = save_obj(str(tmp_path / "out" / "model.obj"), m, save_normal=True, save_uv=True, save_mat=True, map_Kd=kd, map_format="png")
    d = str(tmp_path / "out")
    assert paths == [os.path.join(d, "model.mtl"), os.path.join(d, "texture_kd.png"), os.path.join(d, "model.obj")]
    assert open(paths[0]).read() == "newmtl default\nKa 0.0 0.0 0.0\nmap_Kd texture_kd.png\nKs 0.0 0.0 0.0\n"
    np.testing.assert_array_equal(np.asarray(Image.open(paths[1])), kd.numpy())
    lines = open(paths[2]).read().splitlines()
    assert lines[:3] == ["mtllib model.mtl", "g object", "usemtl default"]
    assert [l.split()[0] for l in lines[3:]] == ["v"] * 4 + ["vn"] * 4 + ["vt"] * 12 + ["f"] * 4
    header, v, vn, vt, f = read_obj_uv(paths[2])
    assert header == lines[:3] and v.shape == (4, 3) and vn.shape == (4, 3)
    np.testing.assert_array_equal(v.astype(np.float32), m.v_pos.numpy())
    np.testing.assert_array_equal(vn.astype(np.float32), m.v_nrm.numpy())
    want_vt = m.v_tex.numpy().astype(np.float64)
    np.testing.assert_array_equal(vt[:, 0], want_vt[:, 0])
    np.testing.assert_allclose(vt[:, 1], 1.0 - want_vt[:, 1], rtol=0, atol=1e-9)        # flipped; %.9g keeps nine digits
    assert lines[3 + 8 + 8] == "vt 0 0.699999988" and lines[3 + 8 + 6] == "vt 0.25 0.875"
    np.testing.assert_array_equal(f[:, :, 0], m.t_pos_idx.numpy() + 1)      # 1-based a/t/a
    np.testing.assert_array_equal(f[:, :, 1], m.t_tex_idx.numpy() + 1)
    np.testing.assert_array_equal(f[:, :, 2], m.t_pos_idx.numpy() + 1)
    assert lines[-4] == "f 1/10/1 3/11/3 2/12/2"

    # without normals `a/t/`; a grey map is written as RGB; every map of the MTL in the reference's order; jpg opens at the right size
    pm = torch.full((4, 4, 1), 200, dtype=torch.uint8)
    paths = save_obj(str(tmp_path / "j" / "m.obj"), m, save_uv=True, save_mat=True, map_Kd=kd, map_Bump=kd, map_Pm=pm, map_Pr=pm[..., 0], map_format="jpg")
    assert [os.path.basename(p) for p in paths] == ["m.mtl", "texture_kd.jpg", "texture_nrm.jpg", "texture_metallic.jpg", "texture_roughness.jpg", "m.obj"]
    assert open(paths[0]).read() == ("newmtl default\nKa 0.0 0.0 0.0\nmap_Kd texture_kd.jpg\nKs 0.0 0.0 0.0\nmap_Bump texture_nrm.jpg\n"
                                     "map_Pm texture_metallic.jpg\nmap_Pr texture_roughness.jpg\n")
    for p in paths[1:5]:
        im = Image.open(p)
        assert im.size == (4, 4) and im.mode == "RGB" and im.format == "JPEG"
    assert open(paths[-1]).read().splitlines()[-4] == "f 1/10/ 3/11/ 2/12/"
    # no albedo: the constant Kd
    paths = save_obj(str(tmp_path / "k" / "m.obj"), m, save_uv=True, save_mat=True)
    assert [os.path.basename(p) for p in paths] == ["m.mtl", "m.obj"]
    assert open(paths[0]).read() == "newmtl default\nKa 0.0 0.0 0.0\nKd 1.0 1.0 1.0\nKs 0.0 0.0 0.0\n"
    # a float map goes through the reference's conversion: clip, * 255, truncate
    paths = save_obj(str(tmp_path / "l" / "m.obj"), m, save_uv=True, save_mat=True, map_Kd=torch.tensor([[[-1.0, 0.5, 2.0]]]), map_format="png")
    assert np.asarray(Image.open(paths[1])).tolist() == [[[0, 127, 255]]]


def test_save_obj_without_uv_is_unchanged(tmp_path):
    from scaledreamer_amd.mesh import save_obj

    m = _textured_tetrahedron()
    m.set_vertex_color(torch.tensor([[0.0, 0.25, 1.0], [0.1, 0.2, 0.3], [1.0, 1.0, 1.0], [1.0 / 3.0, 0.5, 0.75]]))
    path = save_obj(str(tmp_path / "a.obj"), m, save_normal=True, save_vertex_color=True)
    assert path == str(tmp_path / "a.obj")        # the plain call still returns the one path it wrote
    n = m.v_nrm.numpy().astype(np.float64)
    want = ("v 0 0 0 0 0.25 1\nv 1 0 0 0.100000001 0.200000003 0.300000012\nv 0 1 0 1 1 1\nv 0.100000001 0.200000003 0.333333343 0.333333343 0.5 0.75\n"
            + "".join("vn %.9g %.9g %.9g\n" % tuple(r) for r in n) + "f 1//1 3//3 2//2\nf 1//1 2//2 4//4\nf 2//2 3//3 4//4\nf 3//3 1//1 4//4\n")
    assert open(path).read() == want
    assert open(save_obj(str(tmp_path / "b.obj"), m)).read() == ("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0.100000001 0.200000003 0.333333343\n"
                                                                 "f 1// 3// 2//\nf 1// 2// 4//\nf 2// 3// 4//\nf 3// 1// 4//\n")
