"""The per-face UV atlas on the GPU (csrc/atlas.hip): ownership, coverage and texture coordinates against a float64 restatement of the
layout, baked positions against float64 barycentric interpolation, bilinear lookups that never leave their face, the uint8 packing, and
the textured export of an ImplicitVolume end to end."""
import os

import numpy as np
import pytest
import torch

from atlas_util import (barycentric, bilinear_texels, closest_on_triangle, corners_ref, layout_ref, ownership_ref, read_obj_uv,
                        smallest_pow2_texture_size)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def fan_mesh(F, seed=0, scale=1.0):
    """F triangles (0, k + 1, k + 2) over F + 2 seeded random vertices; F = 4 is a tetrahedron"""
    g = torch.Generator().manual_seed(seed)
    if F == 4:
        v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.2, 1.0 / 3.0]]) * scale
        f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    else:
        v = (torch.rand(F + 2, 3, generator=g) * 2.0 - 1.0) * scale
        f = torch.stack([torch.zeros(F, dtype=torch.long), torch.arange(F) + 1, torch.arange(F) + 2], dim=1)
    return v.to(DEV), f.to(DEV)


def bake(v, f, T, g):
    from scaledreamer_amd import ops

    lay = ops.atlas_layout(f.shape[0], T, g)
    v_tex, t_tex_idx = ops.atlas_uv(lay, v.device)
    gb_pos, face_id, covered = ops.atlas_bake(lay, v, f)
    torch.cuda.synchronize()
    return lay, v_tex.cpu().numpy(), t_tex_idx.cpu().numpy(), gb_pos.cpu().numpy(), face_id.cpu().numpy(), covered.cpu().numpy()


def texel_centres(T):
    j, i = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    return np.stack([i + 0.5, j + 0.5], axis=-1).reshape(-1, 2)


# ---- 1. layout edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("T", [16, 50])
@pytest.mark.parametrize("F", [1, 4, 5, 9])
def test_ownership_coverage_and_uv_equal_the_restatement(F, T, g):
    """Triangle corners are integers and texel centres half-integers: every inside test is exact in float64, no texel is excluded."""
    from scaledreamer_amd import _lib, ops

    v, f = fan_mesh(F)
    want = layout_ref(F, T, g)
    if want is None:
        with pytest.raises(_lib.AsdError, match="smallest texture_size that fits"):
            ops.atlas_layout(F, T, g)
        return
    n, c, L = want
    lay, v_tex, t_tex_idx, gb_pos, face_id, covered = bake(v, f, T, g)
    assert (lay.n, lay.c, lay.L) == want
    corners = corners_ref(F, T, g)
    np.testing.assert_array_equal(v_tex, (corners.astype(np.float32) / np.float32(T)))      # exact when T is a power of two, else the rounded quotient
    np.testing.assert_array_equal(t_tex_idx, np.arange(3 * F).reshape(F, 3))
    assert v_tex.min() >= 0.0 and v_tex.max() <= 1.0
    fid = ownership_ref(F, T, g)
    np.testing.assert_array_equal(face_id, fid)
    own = fid.reshape(-1) >= 0
    _, inside = closest_on_triangle(texel_centres(T)[own], corners.reshape(F, 3, 2)[fid.reshape(-1)[own]].astype(np.float64))
    cov = np.zeros(T * T, np.uint8)
    cov[own] = inside
    np.testing.assert_array_equal(covered.reshape(-1), cov)
    assert (gb_pos[face_id < 0] == 0).all()
    # the strip beyond n c, the empty half-cell of an odd F, the cells behind the last face
    assert (face_id[:, n * c:] == -1).all() and (face_id[n * c:, :] == -1).all()
    P = -(-F // 2)
    for k in range(P - 1 if F % 2 else P, n * n):
        cell = face_id[(k // n) * c:(k // n + 1) * c, (k % n) * c:(k % n + 1) * c]
        assert (cell[np.add.outer(np.arange(c), np.arange(c)) + 1 > c] == -1).all()
        if k >= P:
            assert (cell == -1).all()
    for k in range(F):      # every face owns texels, and covers L (L + 1) / 2 of them: the centres with u + v <= L
        assert (face_id == k).sum() == c * (c - 1) // 2 and covered[face_id == k].sum() == L * (L + 1) // 2


# ---- 2. positions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,T,g,scale", [(1, 16, 1, 1.0), (4, 16, 0, 1.0), (5, 64, 2, 100.0), (9, 50, 1, 1.0), (9, 64, 1, 1e-3), (200, 256, 1, 1.0)])
def test_positions_equal_float64_barycentric_interpolation(F, T, g, scale):
    """The reference is float64: the texel centre (covered) or its nearest point on the face's UV triangle (gutter), weights from the
    triangle's corners T v_tex (integers, so rint recovers them exactly), pos = sum_k w_k p_k.
    The kernel computes b_k = w_k * fl(1 / L) from the exact w_k (two roundings: the reciprocal, the product), t_k = p_k * b_k (one),
    (t_0 + t_1) + t_2 (two on corners 0 and 1, one on corner 2), no contraction: pos = sum_k p_k b_k_exact (1 + e_k) with
    |e_k| <= (1 + 2^-24)^5 - 1, and sum_k b_k_exact = 1 with every b_k >= 0, so |pos - exact| <= 5 * 2^-24 * max |p| (1 + 2^-22)
    <= 5 ulps of the largest coordinate (ulp(M) > 2^-24 M).  The float64 reference's own error is below 1e-13 ulp."""
    v, f = fan_mesh(F, seed=F, scale=scale)
    lay, v_tex, t_tex_idx, gb_pos, face_id, covered = bake(v, f, T, g)
    own = face_id.reshape(-1) >= 0
    fid = face_id.reshape(-1)[own]
    tri = np.rint(v_tex.astype(np.float64) * T)[t_tex_idx[fid]]
    q, inside = closest_on_triangle(texel_centres(T)[own], tri)
    np.testing.assert_array_equal(inside, covered.reshape(-1)[own].astype(bool))
    w = barycentric(q, tri)
    assert w.min() >= -1e-12 and np.abs(w.sum(1) - 1).max() < 1e-12
    p = v.cpu().numpy().astype(np.float64)[f.cpu().numpy()[fid]]        # [N, 3 corners, 3]
    want = np.einsum("nk,nkc->nc", w, p)
    M = float(np.abs(v.cpu().numpy()).max())
    bound = 5.0 * float(np.spacing(np.float32(M)))
    err = np.abs(gb_pos.reshape(-1, 3)[own].astype(np.float64) - want)
    gut = ~inside
    print(f"F {F} T {T} g {g}: {own.sum()} owned texels ({gut.sum()} in the gutter), max |gb_pos - float64| = {err.max():.3e} "
          f"= {err.max() / np.spacing(np.float32(M)):.2f} ulp of {M:.4g} (bound 5 ulp = {bound:.3e}); gutter alone {err[gut].max() if gut.any() else 0.0:.3e}")
    assert err.max() <= bound


# ---- 3. no bleeding -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    from scaledreamer_amd.isosurface import MarchingTetrahedraGridHelper, regular_grid_vertices

    res = 17
    p = regular_grid_vertices(res, DEV)
    m = MarchingTetrahedraGridHelper(res).to(DEV)((p - 0.5).norm(dim=-1) - 0.3)
    assert m.t_pos_idx.shape[0] > 500
    return m


def lookups_off_their_face(mesh, g, n_points=100_000):
    """(number of the four-texel lookups at random points of random faces' UV triangles that read a texel of another owner, T)"""
    F = mesh.t_pos_idx.shape[0]
    T = smallest_pow2_texture_size(F, g)
    lay, v_tex, t_tex_idx, _, face_id, _ = bake(mesh.v_pos, mesh.t_pos_idx, T, g)
    rng = np.random.default_rng(7)
    face = rng.integers(0, F, n_points)
    w = rng.dirichlet(np.ones(3), n_points)
    w[:3000] = np.eye(3)[rng.integers(0, 3, 3000)]                      # corners
    edge = rng.random(6000)
    w[3000:9000] = 0.0                                                  # edges: one weight zero
    k = rng.integers(0, 3, 6000)
    w[np.arange(3000, 9000), k] = edge
    w[np.arange(3000, 9000), (k + 1) % 3] = 1.0 - edge
    tri = v_tex.astype(np.float64)[t_tex_idx[face]] * T                 # exact: T is a power of two
    xy = np.einsum("nk,nkc->nc", w, tri)
    j, i = bilinear_texels(xy[:, 0], xy[:, 1], T)
    return int((face_id[j, i] != face[:, None]).any(axis=1).sum()), T


@pytest.mark.parametrize("g", [1, 2])
def test_bilinear_lookups_inside_a_face_read_only_that_face(sphere, g):
    bad, T = lookups_off_their_face(sphere, g)
    print(f"gutter {g}: texture {T}, {sphere.t_pos_idx.shape[0]} faces, {bad} of 100000 lookups read another owner's texel")
    assert bad == 0


def test_without_a_gutter_lookups_do_bleed(sphere):
    bad, T = lookups_off_their_face(sphere, 0)
    print(f"gutter 0: texture {T}, {bad} of 100000 lookups read another owner's texel")
    assert bad > 0, "the check above can fail"


# ---- 4. pack --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_pack_equals_numpy_truncation(C):
    from scaledreamer_amd import ops

    T = 64
    k255 = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    edge = np.concatenate([k255, np.nextafter(k255, np.float32(2)), np.nextafter(k255, np.float32(-1)),
                           np.asarray([-1.0, -0.0, 0.0, 1e-9, -1e-9, 0.5, 0.999999, 1.0, 1.0000001, 2.0, 1e30, -1e30], np.float32)])
    rng = np.random.default_rng(C)
    values = np.concatenate([edge, rng.uniform(-0.2, 1.2, 3000 * C - len(edge) % C).astype(np.float32)])
    values = values[:len(values) // C * C].reshape(-1, C)
    n = len(values)
    assert n < T * T
    index = rng.permutation(T * T)[:n].astype(np.int64)
    image = torch.zeros((T, T, C), dtype=torch.uint8, device=DEV)
    out = ops.atlas_pack_u8(torch.from_numpy(values).to(DEV), torch.from_numpy(index).to(DEV), image)
    assert out is image
    want = np.zeros((T * T, C), np.uint8)
    want[index] = (np.clip(values, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    got = image.cpu().numpy().reshape(T * T, C)
    np.testing.assert_array_equal(got, want)
    untouched = np.ones(T * T, bool)
    untouched[index] = False
    assert untouched.sum() == T * T - n and (got[untouched] == 0).all()
    # an index outside the image writes nothing
    image.zero_()
    ops.atlas_pack_u8(torch.ones(2, C, device=DEV), torch.tensor([-1, T * T], device=DEV), image)
    assert int(image.count_nonzero()) == 0


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
THRESHOLD = 25.0
GUTTER = 1


FEATURE_GAIN = 3.0e4


def make_system(exporter, **geometry):
    """the recipe of test_gpu_mesh.py's `system`: the asd_sd_nerf preset with seeded random weights, no guidance, the density blob raised
    to 60 so that a surface exists at the preset's threshold 25, marching tetrahedra over the regular grid at resolution 32.
    One addition: the hash grid starts at U(-1e-4, 1e-4), so the untrained colour is sigmoid(~1e-5) and EVERY texel truncates to 127 (measured
    on the MI355X: 193920 owned texels, one value) — an 8-bit texture of that field cannot show anything.  The first layer of the FEATURE
    network is scaled by 3e4, which brings the features to O(1) and leaves the density, hence the mesh, as the recipe gives them."""
    from scaledreamer_amd import plugins, presets  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    cfg = presets.asd_sd_nerf()["system"]
    cfg.update(guidance_type="", optimizer={}, exporter=exporter)
    cfg["geometry"].update(density_blob_scale=60.0, isosurface_method="mt-grid", isosurface_resolution=32, isosurface_coarse_to_fine=True,
                           isosurface_threshold=THRESHOLD)
    cfg["geometry"].update(geometry)
    system = find("scaledreamer-system")(cfg).eval()
    with torch.no_grad():
        system.geometry.feature_network.layers[0].weight.mul_(FEATURE_GAIN)
    return system


def test_export_writes_a_textured_obj(tmp_path):
    from PIL import Image

    from scaledreamer_amd import ops

    exporter = {"uv_method": "face-cells", "fmt": "obj-mtl", "texture_format": "png", "save_normal": True, "uv_gutter": GUTTER}
    system = make_system(dict(exporter))
    mesh = system.geometry.isosurface()
    F = mesh.t_pos_idx.shape[0]
    T = smallest_pow2_texture_size(F, GUTTER)
    assert F > 100 and layout_ref(F, T // 2, GUTTER) is None
    n_owned = F * layout_ref(F, T, GUTTER)[1] * (layout_ref(F, T, GUTTER)[1] - 1) // 2      # c (c - 1) / 2 texels per face
    exporter["texture_chunk"] = n_owned // 3 + 1        # three field evaluations, the last one partial
    system.cfg.exporter = dict(exporter, texture_size=T // 2)       # refused by the layout, through the exporter, naming the size that fits
    with pytest.raises(ValueError, match=f"{F} faces do not fit a texture_size of {T // 2} with gutter {GUTTER} .*smallest texture_size that fits is"):
        system.export(str(tmp_path / "small"))
    system.cfg.exporter = dict(exporter, texture_size=T)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    paths = system.export(a)
    assert paths == [os.path.join(a, "model.mtl"), os.path.join(a, "texture_kd.png"), os.path.join(a, "model.obj")]
    assert open(paths[0]).read() == "newmtl default\nKa 0.0 0.0 0.0\nmap_Kd texture_kd.png\nKs 0.0 0.0 0.0\n"
    header, v, vn, vt, f = read_obj_uv(paths[2])
    assert header == ["mtllib model.mtl", "g object", "usemtl default"]
    np.testing.assert_array_equal(v.astype(np.float32), mesh.v_pos.cpu().numpy())
    np.testing.assert_array_equal(f[:, :, 0] - 1, mesh.t_pos_idx.cpu().numpy())
    np.testing.assert_array_equal(f[:, :, 2], f[:, :, 0])
    assert vn.shape == v.shape == (mesh.v_pos.shape[0], 3)
    assert vt.shape == (3 * F, 2) and vt.min() >= 0.0 and vt.max() <= 1.0       # every vt triangle inside the unit square
    np.testing.assert_array_equal(f[:, :, 1] - 1, np.arange(3 * F).reshape(F, 3))

    # the texture against the field at the baked points, in one batch
    lay = ops.atlas_layout(F, T, GUTTER)
    gb_pos, face_id, covered = ops.atlas_bake(lay, mesh.v_pos, mesh.t_pos_idx)
    owned = face_id.view(-1) >= 0
    with torch.no_grad():
        pts = gb_pos.view(-1, 3)[owned]
        albedo = system.material.export(points=pts, **system.geometry.export(points=pts))["albedo"]
    want = (np.clip(albedo.cpu().numpy(), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    img = np.asarray(Image.open(paths[1]))
    assert img.shape == (T, T, 3) and img.dtype == np.uint8
    own = owned.cpu().numpy()
    got = img.reshape(-1, 3)[own]
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert own.sum() == n_owned
    print(f"{F} faces, texture {T}: cells of side {lay.c}, leg {lay.L}; {own.sum()} owned texels ({int(covered.sum())} covered), "
          f"{int((diff > 0).any(axis=1).sum())} differ from the one-batch evaluation, largest difference {diff.max()} count")
    assert diff.max() <= 1      # a field value on a truncation boundary under different batching
    assert (img.reshape(-1, 3)[~own] == 0).all()
    assert got.std() > 0 and len(np.unique(got, axis=0)) > 16, "the texture is not constant"
    # vt is the layout's: the OBJ flips v
    v_tex = ops.atlas_uv(lay, DEV)[0].cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(vt[:, 0].astype(np.float32), v_tex[:, 0].astype(np.float32))
    np.testing.assert_allclose(vt[:, 1], 1.0 - v_tex[:, 1], rtol=0, atol=1e-9)      # %.9g keeps nine digits
    # a second export: the same bytes
    again = system.export(b)
    for p, q in zip(paths, again):
        assert open(p, "rb").read() == open(q, "rb").read(), os.path.basename(p)

    # fmt "obj" with save_uv: vt next to vertex colours, no material
    system.cfg.exporter = {"uv_method": "face-cells", "fmt": "obj", "save_uv": True, "texture_size": T, "uv_gutter": GUTTER}
    (path,) = system.export(str(tmp_path / "c"))
    header, v2, vn2, vt2, f2 = read_obj_uv(path)
    assert header == [] and v2.shape == (mesh.v_pos.shape[0], 6) and vn2.size == 0
    np.testing.assert_array_equal(vt2, vt)
    np.testing.assert_array_equal(f2[:, :, :2], f[:, :, :2])
    assert (f2[:, :, 2] == 0).all()


# ---- 6. no faces ----------------------------------------------------------------------------------------------------------------------
def test_a_level_that_never_crosses_exports_an_empty_mesh(tmp_path):
    from scaledreamer_amd import ops

    lay = ops.atlas_layout(0, 16, 1)
    v_tex, t_tex_idx = ops.atlas_uv(lay, DEV)
    gb_pos, face_id, covered = ops.atlas_bake(lay, torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.long, device=DEV))
    assert v_tex.shape == (0, 2) and t_tex_idx.shape == (0, 3)
    assert bool((face_id == -1).all()) and int(covered.count_nonzero()) == 0 and int(gb_pos.count_nonzero()) == 0
    system = make_system({"uv_method": "face-cells", "fmt": "obj-mtl", "texture_format": "png", "texture_size": 16},
                         isosurface_threshold=1.0e9, isosurface_coarse_to_fine=False)
    paths = system.export(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["model.mtl", "model.obj"]          # nothing owned: no map, the constant Kd
    assert open(paths[0]).read() == "newmtl default\nKa 0.0 0.0 0.0\nKd 1.0 1.0 1.0\nKs 0.0 0.0 0.0\n"
    header, v, vn, vt, f = read_obj_uv(paths[1])
    assert header == ["mtllib model.mtl", "g object", "usemtl default"] and v.size == 0 and vt.shape == (0, 2) and f.shape == (0, 3, 3)
