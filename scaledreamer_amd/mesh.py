"""`Mesh` (threestudio/models/mesh.py:12-160): vertices, faces, extras, vertex normals and colours, outlier removal.

remove_outlier runs on the HIP path (csrc/mesh.hip: connected components by min-label hooking, order-preserving compaction) where the
reference goes through trimesh on the host.  Deviation: components are joined by shared VERTEX, trimesh joins faces by shared edge — the
two differ only where components touch in a single vertex.  UV unwrapping (xatlas) and tangents are not part of this port.
"""
from __future__ import annotations

import os
from typing import Any, Dict, Optional, Union

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

    def _compute_vertex_normal(self) -> torch.Tensor:
        """area-weighted: face normals (un-normalised cross products) splatted to their corners (mesh.py:134-160)"""
        i0, i1, i2 = self.t_pos_idx[:, 0], self.t_pos_idx[:, 1], self.t_pos_idx[:, 2]
        v0, v1, v2 = self.v_pos[i0, :], self.v_pos[i1, :], self.v_pos[i2, :]
        face_normals = torch.cross(v1 - v0, v2 - v0, dim=-1)
        v_nrm = torch.zeros_like(self.v_pos)
        for i in (i0, i1, i2):
            v_nrm.scatter_add_(0, i[:, None].repeat(1, 3), face_normals)
        v_nrm = torch.where((v_nrm * v_nrm).sum(-1, keepdim=True) > 1e-20, v_nrm, torch.as_tensor([0.0, 0.0, 1.0]).to(v_nrm))
        return F.normalize(v_nrm, dim=1)


def save_obj(path: str, mesh: Mesh, save_normal: bool = False, save_vertex_color: bool = False) -> str:
    """The text layout of SaverMixin._save_obj (threestudio/utils/saving.py:501-544) without material or texture coordinates:
    `v x y z [r g b]`, `vn x y z`, `f a//a b//b c//c` (`f a// b// c//` without normals), 1-based.  Lines are formatted per row and joined
    once: the reference's `+=` per vertex is quadratic."""
    import numpy as np

    v = mesh.v_pos.detach().cpu().numpy().astype(np.float64)
    f = mesh.t_pos_idx.detach().cpu().numpy().astype(np.int64) + 1
    if save_vertex_color:
        if mesh.v_rgb is None:
            raise ValueError("save_vertex_color without vertex colours: call mesh.set_vertex_color first")
        v = np.concatenate([v, mesh.v_rgb.detach().cpu().numpy().astype(np.float64)], axis=1)
    # %.9g round-trips every fp32 value
    lines = ["v " + " ".join("%.9g" % x for x in row) for row in v]
    if save_normal:
        lines += ["vn %.9g %.9g %.9g" % tuple(row) for row in mesh.v_nrm.detach().cpu().numpy().astype(np.float64)]
        lines += ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in f]
    else:
        lines += ["f %d// %d// %d//" % (a, b, c) for a, b, c in f]
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path
