"""Mesh extraction on the GPU (csrc/mesh.hip): marching tetrahedra in its explicit and its Kuhn form against the reference's own
MarchingTetrahedraHelper._forward (tests/golden/isosurface_mt_kuhn6.npz), analytic surfaces, run-to-run identity, the scan across blocks,
connected components against scipy, and the export of an ImplicitVolume end to end.

Meshes are compared in canonical form (mesh_util.canonical): vertices sorted by coordinate, faces re-indexed, rotated to their smallest
index and sorted — winding is significant, vertex and face order are not.
"""
import os

import numpy as np
import pytest
import torch

from mesh_util import canonical, canonical_faces, edge_stats, read_obj, signed_volume

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isosurface_mt_kuhn6.npz")
FIELDS = ["sphere", "two_spheres", "torus", "noise"]
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


_explicit_helpers = {}


def explicit_helper(res):
    """the Kuhn grid as a MarchingTetrahedraHelper over explicit arrays built with tensor ops on the device, one per resolution"""
    from scaledreamer_amd.isosurface import MarchingTetrahedraHelper, kuhn_tet_indices, regular_grid_vertices

    if res not in _explicit_helpers:
        _explicit_helpers[res] = MarchingTetrahedraHelper(res, vertices=regular_grid_vertices(res, DEV), indices=kuhn_tet_indices(res, DEV)).to(DEV)
    return _explicit_helpers[res]


def grid_helper(res):
    from scaledreamer_amd.isosurface import MarchingTetrahedraGridHelper

    return MarchingTetrahedraGridHelper(res).to(DEV)


def np_mesh(mesh):
    return mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy()


def field_points(res, bbox=(-1.0, 1.0)):
    from scaledreamer_amd.isosurface import regular_grid_vertices

    return regular_grid_vertices(res, DEV) * (bbox[1] - bbox[0]) + bbox[0]


def sphere_level(p, centre, r):
    return (p - torch.as_tensor(centre, device=p.device, dtype=p.dtype)).norm(dim=-1) - r


def torus_level(p, R, r):
    return torch.sqrt((torch.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def extra_fields(res):
    """the golden's four kinds of field at another resolution"""
    p = field_points(res, (0.0, 1.0))
    c = (0.5, 0.5, 0.5)
    return {"sphere": sphere_level(p, c, 0.3),
            "two_spheres": torch.minimum(sphere_level(p, (0.25, 0.3, 0.3), 0.18), sphere_level(p, (0.75, 0.7, 0.7), 0.15)),
            "torus": torus_level(p - torch.tensor(c, device=DEV), 0.28, 0.12),
            "noise": torch.randn(res**3, generator=torch.Generator().manual_seed(res)).to(DEV)}


# ---- 1. explicit form against the golden --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_explicit_form_equals_the_reference(golden, name):
    """Faces identical in canonical form.  The vertex arithmetic is the reference's three fp32 operations (negate-add, IEEE division,
    multiply-add without contraction), so 8 ulps of the grid extent would be the bound; the difference measured on the MI355X is ZERO for
    all four fields, and the test asks for equality."""
    from scaledreamer_amd.isosurface import MarchingTetrahedraHelper

    h = MarchingTetrahedraHelper(int(golden["res"]), vertices=golden["verts"], indices=golden["tet_verts"].astype(np.int64)).to(DEV)
    np.testing.assert_array_equal(h.all_edges.cpu().numpy(), golden["edges"])
    np.testing.assert_array_equal(h._edge_tables()[3].cpu().numpy(), golden["tet_edges"])
    mesh = h(torch.from_numpy(golden[f"{name}.level"]).to(DEV))
    v, f = np_mesh(mesh)
    rv, rf = golden[f"{name}.verts"], golden[f"{name}.faces"]
    assert v.shape == rv.shape and f.shape == rf.shape and mesh.t_pos_idx.dtype == torch.long
    cv, cf = canonical(v, f)
    crv, crf = canonical(rv, rf)
    print(f"{name}: {len(v)} vertices, {len(f)} faces, max |v - v_ref| = {np.abs(cv - crv).max():.3e} (bound {8 * 2.0**-23:.3e})")
    np.testing.assert_array_equal(cf, crf)
    np.testing.assert_array_equal(cv, crv)
    np.testing.assert_array_equal(v, rv)        # and in the reference's own order: edge order is the order of its torch.unique
    assert set(mesh.extras) >= {"grid_vertices", "grid_level", "tet_edges"}


# ---- 2. Kuhn form against the explicit form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [6, 9])
def test_kuhn_form_equals_the_explicit_form(golden, res):
    """carries the closed-form indexing: non-power-of-two strides, boundary vertices that own fewer than seven edges"""
    fields = {k: torch.from_numpy(golden[f"{k}.level"]).to(DEV) for k in FIELDS} if res == 6 else extra_fields(res)
    kuhn, explicit = grid_helper(res), explicit_helper(res)
    assert torch.equal(kuhn.grid_vertices, explicit.grid_vertices) and kuhn.points_range == (0, 1)
    for name, level in fields.items():
        a, b = kuhn(level), explicit(level)
        assert a.v_pos.shape[0] > 0 and a.t_pos_idx.shape[0] > 0, name
        (av, af), (bv, bf) = canonical(*np_mesh(a)), canonical(*np_mesh(b))
        assert av.tobytes() == bv.tobytes() and af.tobytes() == bf.tobytes(), name
        assert torch.equal(a.v_pos, b.v_pos) and torch.equal(a.t_pos_idx, b.t_pos_idx), name      # slot order is edge order and tet order
        assert torch.equal(a.extras["grid_level"], level) and torch.equal(a.extras["grid_vertices"], kuhn.grid_vertices)
    if res == 6:
        for name in FIELDS:     # and so the Kuhn form equals the reference
            v, f = np_mesh(kuhn(fields[name]))
            np.testing.assert_array_equal(canonical_faces(f), canonical_faces(golden[f"{name}.faces"]))


def test_kuhn_deformation_warns_and_is_ignored(golden, caplog):
    level = torch.from_numpy(golden["sphere.level"]).to(DEV)
    h = grid_helper(6)
    with caplog.at_level("WARNING", logger="scaledreamer_amd"):
        m = h(level, deformation=torch.ones(216, 3, device=DEV))
    assert "does not support deformation" in caplog.text and torch.equal(m.v_pos, h(level).v_pos)
    e = explicit_helper(6)
    moved = e(level, deformation=torch.full((216, 3), 0.3, device=DEV))
    assert not torch.equal(moved.v_pos, e(level).v_pos) and moved.extras["grid_deformation"] is not None


# ---- 3. analytic properties -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analytic():
    res = 33
    p = field_points(res)
    h = grid_helper(res)
    out = {}
    for name, level in (("sphere", sphere_level(p, (0.0, 0.0, 0.0), 0.5)), ("torus", torus_level(p, 0.55, 0.2))):
        m = h(level)
        out[name] = (m.v_pos.cpu().numpy().astype(np.float64) * 2.0 - 1.0, m.t_pos_idx.cpu().numpy())
    return out


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_analytic_surfaces_are_closed_oriented_manifolds(analytic, name, euler):
    v, f = analytic[name]
    twice_directed, not_two_faces, n_edges = edge_stats(f)
    assert twice_directed == 0, "every directed edge occurs once"
    assert not_two_faces == 0, "every undirected edge lies in exactly two faces"
    assert len(v) - n_edges + len(f) == euler
    assert f.min() == 0 and f.max() == len(v) - 1


def test_sphere_vertices_lie_within_the_interpolation_bound(analytic, golden):
    """A vertex lies on a tet edge of length <= L = sqrt(3) h at the zero of the linear interpolant of f = |x| - r.  Along the edge f'' is at
    most 1 / rho with rho >= r - L the distance of the edge from the centre, so the interpolant is off by at most L^2 / (8 (r - L)), and f
    has slope <= 1 along any line: | |v| - r | <= L^2 / (8 (r - L))."""
    v, f = analytic["sphere"]
    r, L = 0.5, np.sqrt(3.0) * 2.0 / 32
    err = np.abs(np.linalg.norm(v, axis=1) - r).max()
    print(f"sphere res 33: {len(v)} vertices, max | |v| - r | = {err:.3e}, bound {L * L / (8 * (r - L)):.3e}")
    assert err <= L * L / (8 * (r - L))
    ref = signed_volume(golden["sphere.verts"], golden["sphere.faces"])
    vol = signed_volume(v, f)
    assert ref != 0 and np.sign(vol) == np.sign(ref), "wound as the reference winds the golden sphere"
    assert abs(abs(vol) - 4.0 / 3.0 * np.pi * r**3) < 0.05 * 4.0 / 3.0 * np.pi * r**3


# ---- 4. run-to-run identity -------------------------------------------------------------------------------------------------------
def test_two_runs_are_equal_as_raw_tensors():
    level = torch.randn(33**3, generator=torch.Generator().manual_seed(4)).to(DEV)
    h = grid_helper(33)
    a, b = h(level), h(level)
    assert a.v_pos.shape[0] > 10000
    assert torch.equal(a.v_pos, b.v_pos) and torch.equal(a.t_pos_idx, b.t_pos_idx)


# ---- 5. the scan across blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", ["last", "first"])
def test_scan_carries_across_many_blocks(slab):
    """res 65: 7 65^3 = 1.9 M edge slots, 939 scan tiles.  The crossings sit in one z-slab only, so every offset behind (last slab) or in
    front of (first slab) almost all tiles comes from the tile sums alone."""
    from scaledreamer_amd import ops

    res = 65
    k = torch.arange(res, device=DEV).expand(res, res, res)
    inside = (k == res - 1) if slab == "last" else (k == 0)
    level = torch.where(inside, 1.0, -1.0).reshape(-1) * (1.0 + torch.rand(res**3, generator=torch.Generator().manual_seed(5)).to(DEV))
    lay = ops.mt_layout(res)
    assert lay.n_edge_slots == 7 * res**3 and -(-lay.n_edge_slots // 2048) > 900
    a, b = grid_helper(res)(level), explicit_helper(res)(level)
    # the slab z = const of (res - 1)^2 cells: edges along z, the yz / xz face diagonals and the body diagonal cross, and only those
    n_cross = res * res + 2 * res * (res - 1) + (res - 1) ** 2
    assert a.v_pos.shape[0] == b.v_pos.shape[0] == n_cross
    assert a.t_pos_idx.shape[0] == b.t_pos_idx.shape[0] > 0
    assert torch.equal(a.v_pos, b.v_pos) and torch.equal(a.t_pos_idx, b.t_pos_idx)
    z = a.v_pos[:, 2]
    lo, hi = ((res - 2) / (res - 1), 1.0) if slab == "last" else (0.0, 1.0 / (res - 1))
    assert float(z.min()) >= lo - 1e-6 and float(z.max()) <= hi + 1e-6
    assert int(a.t_pos_idx.min()) == 0 and int(a.t_pos_idx.max()) == n_cross - 1
    assert edge_stats(a.t_pos_idx.cpu().numpy())[0] == 0


def test_scan_entry_equals_cumsum():
    from scaledreamer_amd import ops

    g = torch.Generator().manual_seed(6)
    for n in (0, 1, 7, 2047, 2048, 2049, 3 * 2048 + 5, 1024 * 2048 + 1025):       # tile edges, and more tile sums than one trip of their scan
        c = torch.randint(0, 5, (n,), generator=g, dtype=torch.int32).to(DEV)
        off, total = ops.scan_i32_blocks(c)
        want = torch.cumsum(c.long(), 0)
        assert int(total) == (int(want[-1]) if n else 0)
        assert torch.equal(off.long(), want - c.long()), n


# ---- 6. components ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_spheres():
    p = field_points(33)
    level = torch.minimum(sphere_level(p, (-0.4, 0.0, 0.0), 0.45), sphere_level(p, (0.6, 0.5, 0.0), 0.12))
    m = grid_helper(33)(level)
    m.v_pos = m.v_pos * 2.0 - 1.0
    v, f = np_mesh(m)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n_comp, lab = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(len(v), len(v))), directed=False)
    first = np.full(n_comp, len(v))
    np.minimum.at(first, lab, np.arange(len(v)))
    return m, v, f, first[lab], n_comp


def expected_removal(v, f, label, threshold):
    counts = np.bincount(label[f[:, 0]], minlength=len(v))
    thr = int(counts.max() * threshold) if isinstance(threshold, float) else threshold
    vk, fk = counts[label] >= thr, counts[label[f[:, 0]]] >= thr
    remap = np.cumsum(vk) - 1
    return v[vk], remap[f[fk]], counts


def test_component_labels_equal_scipy(two_spheres):
    m, v, f, label, n_comp = two_spheres
    labels, counts = m.components()
    assert n_comp == 2
    np.testing.assert_array_equal(labels.cpu().numpy(), label)      # the smallest vertex index of the component, by either route
    want = np.bincount(label[f[:, 0]], minlength=len(v))
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    ratio = np.sort(want[want > 0])
    print(f"two spheres res 33: {len(v)} vertices, faces per component {ratio.tolist()}, ratio {ratio[0] / ratio[1]:.3f}")
    assert 0.04 < ratio[0] / ratio[1] < 0.10


@pytest.mark.parametrize("threshold,n_kept", [(0.01, 2), (0.2, 1), (50, 2)])
def test_outlier_removal_equals_the_threshold_rule_on_scipy_components(two_spheres, threshold, n_kept):
    m, v, f, label, _ = two_spheres
    m.add_extra("bbox", "kept")
    clean = m.remove_outlier(threshold)
    wv, wf, counts = expected_removal(v, f, label, threshold)
    assert (len(wf) == len(f)) == (n_kept == 2) and len(wf) > 0
    np.testing.assert_array_equal(clean.v_pos.cpu().numpy(), wv)
    np.testing.assert_array_equal(clean.t_pos_idx.cpu().numpy(), wf)
    assert clean.extras is m.extras and clean.t_pos_idx.dtype == torch.long
    assert edge_stats(clean.t_pos_idx.cpu().numpy())[:2] == (0, 0)


def test_isolated_vertex_survives_compaction(two_spheres):
    from scaledreamer_amd.mesh import Mesh

    m, v, f, label, _ = two_spheres
    lone = torch.tensor([[9.0, 9.0, 9.0]], device=DEV)
    for at in (0, len(v)):      # in front of every referenced vertex, and behind them
        vp = torch.cat([lone, m.v_pos]) if at == 0 else torch.cat([m.v_pos, lone])
        tf = m.t_pos_idx + (1 if at == 0 else 0)
        mesh = Mesh(vp, tf)
        labels, counts = mesh.components()
        assert int(labels[at]) == at and int(counts[at]) == 0
        for threshold, lone_kept in ((0.2, False), (0, True)):
            c = mesh.remove_outlier(threshold)
            nv = c.v_pos.shape[0]
            assert int(c.t_pos_idx.min()) >= 0 and int(c.t_pos_idx.max()) < nv
            assert bool((c.v_pos == 9.0).all(dim=1).any()) == lone_kept
            wv, wf, _ = expected_removal(vp.cpu().numpy(), tf.cpu().numpy(), labels.cpu().numpy(), threshold)
            np.testing.assert_array_equal(c.v_pos.cpu().numpy(), wv)
            np.testing.assert_array_equal(c.t_pos_idx.cpu().numpy(), wf)
            referenced = np.unique(c.t_pos_idx.cpu().numpy())
            assert len(referenced) == nv - int(lone_kept)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------
THRESHOLD = 25.0


@pytest.fixture(scope="module")
def system():
    """the asd_sd_nerf preset's geometry / material / background with seeded random weights, no guidance; the density blob is raised
    (scale 60 at the centre, falling to 25 at |x| = 0.29) so that a surface exists at the preset's threshold 25"""
    from scaledreamer_amd import plugins, presets  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    cfg = presets.asd_sd_nerf()["system"]
    cfg.update(guidance_type="", optimizer={}, exporter={"fmt": "obj", "save_uv": False, "save_normal": True})
    cfg["geometry"].update(density_blob_scale=60.0, isosurface_method="mt-grid", isosurface_resolution=32, isosurface_coarse_to_fine=True,
                           isosurface_threshold=THRESHOLD)
    return find("scaledreamer-system")(cfg).eval()


def test_isosurface_of_an_implicit_volume(system):
    from scaledreamer_amd.isosurface import kuhn_grid_arrays

    geo = system.geometry
    assert geo.fused, "the field of the grid vertices is the fused density kernel"
    with torch.no_grad():
        coarse_field = geo.forward_density(field_points(32))
    print(f"field over the coarse grid: min {float(coarse_field.min()):.3f}, max {float(coarse_field.max()):.3f}, threshold {THRESHOLD}")
    assert float(coarse_field.min()) < THRESHOLD < float(coarse_field.max()), "the field crosses the threshold"
    mesh = geo.isosurface()
    nv, nf = mesh.v_pos.shape[0], mesh.t_pos_idx.shape[0]
    assert nv > 100 and nf > 100 and int(mesh.t_pos_idx.max()) < nv and not mesh.requires_grad
    assert bool((mesh.v_pos >= geo.bbox[0]).all()) and bool((mesh.v_pos <= geo.bbox[1]).all())
    box = mesh.extras["bbox"]
    assert bool((box[1] - box[0] < 2.0).all()), "the second pass ran over the tight box"
    assert bool((mesh.v_pos >= box[0] - 1e-6).all()) and bool((mesh.v_pos <= box[1] + 1e-6).all())
    # a vertex is the zero of the linear interpolant of the level along ONE fine tet edge, so the field itself is off the threshold by no
    # more than it changes over such an edge: the largest |d_a - d_b| over the crossing edges of the fine grid, from the field's own values
    level = mesh.extras["grid_level"].reshape(-1)
    edges = kuhn_grid_arrays(32, DEV)[1]
    la, lb = level[edges[:, 0]], level[edges[:, 1]]
    cross = (la > 0) != (lb > 0)
    tol = float((la - lb).abs()[cross].max())
    with torch.no_grad():
        err = float((geo.forward_density(mesh.v_pos) - THRESHOLD).abs().max())
    print(f"fine mesh: {nv} vertices, {nf} faces, max |density(v) - threshold| = {err:.4f}, largest change over a crossing edge {tol:.4f}")
    assert err <= tol
    again = geo.isosurface()
    assert torch.equal(again.v_pos, mesh.v_pos) and torch.equal(again.t_pos_idx, mesh.t_pos_idx)


def test_export_writes_an_obj(system, tmp_path):
    mesh = system.geometry.isosurface()
    paths = system.export(str(tmp_path))
    assert paths == [os.path.join(str(tmp_path), "model.obj")] and os.path.exists(paths[0])
    v, vn, f = read_obj(paths[0])
    assert v.shape == (mesh.v_pos.shape[0], 6) and vn.shape == (mesh.v_pos.shape[0], 3) and f.shape == (mesh.t_pos_idx.shape[0], 3, 3)
    np.testing.assert_array_equal(v[:, :3].astype(np.float32), mesh.v_pos.cpu().numpy())
    np.testing.assert_array_equal(f[:, :, 0] - 1, mesh.t_pos_idx.cpu().numpy())
    assert v[:, 3:].min() >= 0.0 and v[:, 3:].max() <= 1.0 and v[:, 3:].std() > 0


def test_auto_threshold_and_single_pass(system):
    geo = system.geometry
    saved = (geo.cfg.isosurface_threshold, geo.cfg.isosurface_coarse_to_fine, geo.cfg.isosurface_chunk)
    geo.cfg.isosurface_threshold, geo.cfg.isosurface_coarse_to_fine, geo.cfg.isosurface_chunk = "auto", False, 10000
    try:
        mesh = geo.isosurface()
    finally:
        geo.cfg.isosurface_threshold, geo.cfg.isosurface_coarse_to_fine, geo.cfg.isosurface_chunk = saved
    assert mesh.v_pos.shape[0] > 100 and torch.equal(mesh.extras["bbox"], geo.bbox)
