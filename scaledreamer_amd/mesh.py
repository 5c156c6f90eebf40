"""`Mesh` (threestudio/models/mesh.py:12-160): vertices, faces, extras, vertex normals and colours, outlier removal.

remove_outlier runs on the HIP path (csrc/mesh.hip: connected components by min-label hooking, order-preserving compaction) where the
reference goes through trimesh on the host.  Deviation: components are joined by shared VERTEX, trimesh joins faces by shared edge — the
two differ only where components touch in a single vertex.

unwrap_uv does not run xatlas (which this port does not have) but lays out a per-face atlas on the HIP path (csrc/atlas.hip, method
"face-cells"): every face gets a triangle of its own in a grid of square cells, two faces per cell.  That is NOT xatlas's result: there are
3 F texture vertices, no charts, and every face gets the same number of texels whatever its area.  Tangents are not part of this port.
save_obj writes the OBJ, and with a material the MTL and its texture images, in the text layout of SaverMixin._save_obj / _save_mtl.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Union

import torch
import torch.nn.functional as F

from .registry import debug


def outlier_face_threshold(max_component_faces: int, outlier_n_faces_threshold: Union[int, float]) -> int:
    """mesh.py:55-63: a float is a fraction of the largest component's face count, an int the face count itself"""
    if isinstance(outlier_n_faces_threshold, float):
        return int(max_component_faces * outlier_n_faces_threshold)
    return int(outlier_n_faces_threshold)


class Mesh:
    def __init__(self, v_pos: torch.Tensor, t_pos_idx: torch.Tensor, **kwargs) -> None:
        self.v_pos = v_pos
        self.t_pos_idx = t_pos_idx
        self._v_nrm: Optional[torch.Tensor] = None
        self._v_rgb: Optional[torch.Tensor] = None
        self._v_tex: Optional[torch.Tensor] = None
        self._t_tex_idx: Optional[torch.Tensor] = None
        self.atlas = None       # the _lib.AtlasLayout of unwrap_uv: what a bake of this mesh's texture has to use
        self.extras: Dict[str, Any] = {}
        for k, v in kwargs.items():
            self.add_extra(k, v)

    def add_extra(self, k, v) -> None:
        self.extras[k] = v

    @property
    def requires_grad(self) -> bool:
        return self.v_pos.requires_grad

    def components(self):
        """(labels [Nv] int32: the smallest vertex index of each vertex's component, counts [Nv] int32: faces per label)"""
        from . import ops

        return ops.mesh_components(self.t_pos_idx, self.v_pos.shape[0])

    def remove_outlier(self, outlier_n_faces_threshold: Union[int, float]) -> "Mesh":
        if self.requires_grad:
            debug("Mesh is differentiable, not removing outliers")
            return self
        from . import ops

        if self.t_pos_idx.shape[0] == 0:
            return self
        labels, counts = self.components()
        n_faces_threshold = outlier_face_threshold(int(counts.max().item()), outlier_n_faces_threshold)
        debug("Removing components with less than %d faces", n_faces_threshold)
        v_pos, t_pos_idx = ops.mesh_keep_components(self.v_pos, self.t_pos_idx, labels, counts, n_faces_threshold)
        clean_mesh = Mesh(v_pos.to(self.v_pos.dtype), t_pos_idx.to(self.t_pos_idx.dtype))
        if len(self.extras) > 0:        # keep the extras unchanged (mesh.py:89-93)
            clean_mesh.extras = self.extras
        return clean_mesh

    @property
    def v_nrm(self) -> torch.Tensor:
        if self._v_nrm is None:
            self._v_nrm = self._compute_vertex_normal()
        return self._v_nrm

    @property
    def v_rgb(self) -> Optional[torch.Tensor]:
        return self._v_rgb

    def set_vertex_color(self, v_rgb: torch.Tensor) -> None:
        assert v_rgb.shape[0] == self.v_pos.shape[0]
        self._v_rgb = v_rgb

    @property
    def v_tex(self) -> torch.Tensor:
        if self._v_tex is None:
            self.unwrap_uv()
        return self._v_tex

    @property
    def t_tex_idx(self) -> torch.Tensor:
        if self._t_tex_idx is None:
            self.unwrap_uv()
        return self._t_tex_idx

    def set_uv(self, v_tex: torch.Tensor, t_tex_idx: torch.Tensor) -> None:
        """texture coordinates from elsewhere: v_tex [Nt,2] in [0,1]^2, t_tex_idx [Nf,3] into it"""
        assert v_tex.shape[-1] == 2 and tuple(t_tex_idx.shape) == tuple(self.t_pos_idx.shape)
        self._v_tex, self._t_tex_idx, self.atlas = v_tex, t_tex_idx, None

    def unwrap_uv(self, method: str = "face-cells", gutter: int = 1, texture_size: int = 1024) -> None:
        """mesh.py:244-250, with the atlas of csrc/atlas.hip in place of xatlas: sets v_tex [3F,2] and t_tex_idx [F,3].  The layout depends on
        texture_size and gutter (ops.atlas_layout refuses, naming the smallest texture_size, when the faces do not fit)."""
        if method != "face-cells":
            raise ValueError(f'unwrap_uv method {method!r}: only "face-cells" is implemented (xatlas is not part of this port)')
        from . import ops
        from ._lib import AsdError

        try:
            self.atlas = ops.atlas_layout(self.t_pos_idx.shape[0], texture_size, gutter)
        except AsdError as e:       # the faces do not fit: a matter of the configuration
            raise ValueError(str(e)) from e
        self._v_tex, self._t_tex_idx = ops.atlas_uv(self.atlas, self.v_pos.device)

    def _compute_vertex_normal(self) -> torch.Tensor:
        """area-weighted: face normals (un-normalised cross products) splatted to their corners (mesh.py:134-160)"""
        i0, i1, i2 = self.t_pos_idx[:, 0], self.t_pos_idx[:, 1], self.t_pos_idx[:, 2]
        v0, v1, v2 = self.v_pos[i0, :], self.v_pos[i1, :], self.v_pos[i2, :]
        face_normals = torch.cross(v1 - v0, v2 - v0, dim=-1)
        # A scatter_add_ of the corners is a float atomic on the device: the order of the additions, and with it the last bits of a normal,
        # changes from run to run, and two exports of one mesh would differ in their `vn` lines.  Here the corners are sorted by vertex
        # (stable), and round r adds the r-th corner of every vertex: no vertex twice in a round, the same order every run.
        nv = self.v_pos.shape[0]
        v_nrm = torch.zeros_like(self.v_pos)
        corner = self.t_pos_idx.t().reshape(-1)
        if corner.shape[0] > 0:
            order = torch.sort(corner, stable=True).indices
            vertex, normal = corner[order], face_normals.repeat(3, 1)[order]
            counts = torch.bincount(corner, minlength=nv)
            rank = torch.arange(corner.shape[0], device=corner.device) - (torch.cumsum(counts, 0) - counts)[vertex]
            for r in range(int(counts.max())):
                m = rank == r
                v_nrm[vertex[m]] += normal[m]
        v_nrm = torch.where((v_nrm * v_nrm).sum(-1, keepdim=True) > 1e-20, v_nrm, torch.as_tensor([0.0, 0.0, 1.0]).to(v_nrm))
        return F.normalize(v_nrm, dim=1)


def _save_map(path: str, img, map_format: str) -> str:
    """one texture image, uint8 [H,W,3] or [H,W,1] (written as grey RGB, get_grayscale_image_ with cmap None).  JPEG at quality 95, cv2.imwrite's
    default; PNG as it is."""
    import numpy as np
    from PIL import Image

    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8:     # get_rgb_image_ (saving.py:82-86): clip, scale, truncate
        a = (a.clip(0.0, 1.0) * 255.0).astype(np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[-1] == 1:
        a = np.repeat(a, 3, axis=2)
    kw = {"quality": 95} if map_format.lower() in ("jpg", "jpeg") else {}
    Image.fromarray(np.ascontiguousarray(a[..., :3])).save(path, **kw)
    return path


def _save_mtl(path: str, matname: str, maps: Dict[str, Any], map_format: str, Ka=(0.0, 0.0, 0.0), Kd=(1.0, 1.0, 1.0), Ks=(0.0, 0.0, 0.0)) -> List[str]:
    """SaverMixin._save_mtl (saving.py:546-641), line for line: newmtl, Ka, map_Kd | Kd, map_Ks | Ks, map_Bump, map_Pm, map_Pr"""
    here = os.path.dirname(path)
    paths = [path]
    lines = [f"newmtl {matname}", f"Ka {Ka[0]} {Ka[1]} {Ka[2]}"]
    for key, stem, constant in (("map_Kd", "texture_kd", f"Kd {Kd[0]} {Kd[1]} {Kd[2]}"), ("map_Ks", "texture_ks", f"Ks {Ks[0]} {Ks[1]} {Ks[2]}"),
                                ("map_Bump", "texture_nrm", None), ("map_Pm", "texture_metallic", None), ("map_Pr", "texture_roughness", None)):
        if maps.get(key) is not None:
            lines.append(f"{key} {stem}.{map_format}")
            paths.append(_save_map(os.path.join(here, f"{stem}.{map_format}"), maps[key], map_format))
        elif constant is not None:
            lines.append(constant)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return paths


def save_obj(path: str, mesh: Mesh, save_normal: bool = False, save_vertex_color: bool = False, save_uv: bool = False, save_mat: bool = False,
             map_Kd=None, map_Ks=None, map_Bump=None, map_Pm=None, map_Pr=None, map_format: str = "jpg") -> Union[str, List[str]]:
    """The text layout of SaverMixin._save_obj (threestudio/utils/saving.py:501-544): `mtllib`, `g object`, `usemtl default` with a material,
    `v x y z [r g b]`, `vn x y z`, `vt u 1-v`, `f a/t/a b/t/b c/t/c` (`f a/t/` without normals, `f a//a` and `f a//` without texture
    coordinates), 1-based.  Lines are formatted per row and joined once: the reference's `+=` per vertex is quadratic.
    save_mat writes <name>.mtl and the given maps (uint8 or [0,1] float, [H,W,3] or [H,W,1]) next to the OBJ first.
    Returns the OBJ's path; with save_mat every written path as the reference's save_obj does: the MTL, its textures, the OBJ last."""
    import numpy as np

    paths: List[str] = []
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    lines: List[str] = []
    if save_mat:
        mtl = path[:-len(".obj")] + ".mtl" if path.endswith(".obj") else path + ".mtl"
        paths += _save_mtl(mtl, "default", {"map_Kd": map_Kd, "map_Ks": map_Ks, "map_Bump": map_Bump, "map_Pm": map_Pm, "map_Pr": map_Pr}, map_format)
        lines += [f"mtllib {os.path.basename(mtl)}", "g object", "usemtl default"]
    v = mesh.v_pos.detach().cpu().numpy().astype(np.float64)
    f = mesh.t_pos_idx.detach().cpu().numpy().astype(np.int64) + 1
    if save_vertex_color:
        if mesh.v_rgb is None:
            raise ValueError("save_vertex_color without vertex colours: call mesh.set_vertex_color first")
        v = np.concatenate([v, mesh.v_rgb.detach().cpu().numpy().astype(np.float64)], axis=1)
    # %.9g round-trips every fp32 value
    lines += ["v " + " ".join("%.9g" % x for x in row) for row in v]
    if save_normal:
        lines += ["vn %.9g %.9g %.9g" % tuple(row) for row in mesh.v_nrm.detach().cpu().numpy().astype(np.float64)]
    if save_uv:
        vt = mesh.v_tex.detach().cpu().numpy().astype(np.float64)
        ft = mesh.t_tex_idx.detach().cpu().numpy().astype(np.int64) + 1
        lines += ["vt %.9g %.9g" % (u, 1.0 - w) for u, w in vt]
        if save_normal:
            lines += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, ta, a, b, tb, b, c, tc, c) for (a, b, c), (ta, tb, tc) in zip(f, ft)]
        else:
            lines += ["f %d/%d/ %d/%d/ %d/%d/" % (a, ta, b, tb, c, tc) for (a, b, c), (ta, tb, tc) in zip(f, ft)]
    elif save_normal:
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in f]
    else:
        lines += ["f %d// %d// %d//" % (a, b, c) for a, b, c in f]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    paths.append(path)
    return paths if save_mat else path
