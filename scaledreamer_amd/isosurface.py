"""Isosurface helpers (threestudio/models/isosurface.py:11-253) on the HIP path: marching tetrahedra over a tets file (`mt`, the
reference's MarchingTetrahedraHelper) or over the Kuhn subdivision of a regular grid (`mt-grid`, no file).  The kernels are
csrc/mesh.hip (ops.marching_tetrahedra); the tables of the explicit form depend on the grid alone and are built once with tensor ops,
as the reference's `all_edges` is.  There are no marching cubes here (`mc-cpu` needs PyMCubes).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .mesh import Mesh
from .registry import warn

# the six tetrahedra of a cell as corner codes (di dj dk): csrc/mesh.hip kuhn_tet — all wound with det[v1-v0, v2-v0, v3-v0] > 0
KUHN_TETS = ((0, 4, 6, 7), (0, 5, 4, 7), (0, 6, 2, 7), (0, 2, 3, 7), (0, 1, 5, 7), (0, 3, 1, 7))
BASE_TET_EDGES = (0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3)


def regular_grid_vertices(resolution: int, device=None) -> torch.Tensor:
    """linspace(0,1,res)^3, `ij` order (MarchingCubeCPUHelper.grid_vertices, isosurface.py:32-46)"""
    t = torch.linspace(0, 1, resolution, device=device)
    x, y, z = torch.meshgrid(t, t, t, indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], dim=-1)


def kuhn_tet_indices(resolution: int, device=None) -> torch.Tensor:
    """[6 (res-1)^3, 4] int64: tet 6 c + t of cell c = (i (res-1) + j) (res-1) + k, vertices numbered (i res + j) res + k"""
    r = resolution
    c = torch.arange(r - 1, device=device)
    i, j, k = torch.meshgrid(c, c, c, indexing="ij")
    base = ((i * r + j) * r + k).reshape(-1, 1, 1)
    code = torch.as_tensor(KUHN_TETS, device=device)
    off = ((code >> 2) & 1) * r * r + ((code >> 1) & 1) * r + (code & 1)
    return (base + off[None]).reshape(-1, 4)


def tet_edge_tables(indices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(edges [Ne,2] unique, a < b, sorted: the reference's all_edges (isosurface.py:143-156); tet_edges [Nt,6]: the row of `edges` of every
    tet's edges 01 02 03 12 13 23), int64"""
    e = indices[:, torch.as_tensor(BASE_TET_EDGES, device=indices.device)].reshape(-1, 2)
    e = torch.sort(e, dim=1)[0]
    edges, inverse = torch.unique(e, dim=0, return_inverse=True)
    return edges, inverse.reshape(-1, 6)


def kuhn_grid_arrays(resolution: int, device=None):
    """the `mt-grid` grid as explicit arrays: (verts [res^3,3], edges, tet_verts, tet_edges)"""
    tets = kuhn_tet_indices(resolution, device)
    edges, tet_edges = tet_edge_tables(tets)
    return regular_grid_vertices(resolution, device), edges, tets, tet_edges


class IsosurfaceHelper(nn.Module):
    points_range: Tuple[float, float] = (0, 1)

    @property
    def grid_vertices(self) -> torch.Tensor:
        raise NotImplementedError


class MarchingTetrahedraHelper(IsosurfaceHelper):
    """explicit form: a tets file with `vertices` [Nv,3] and `indices` [Nt,4] (load/tets/{res}_tets.npz), or the two arrays themselves"""

    def __init__(self, resolution: int, tets_path: Optional[str] = None, vertices=None, indices=None):
        super().__init__()
        self.resolution = resolution
        self.tets_path = tets_path
        if tets_path is not None:
            tets = np.load(tets_path)
            vertices, indices = tets["vertices"], tets["indices"]
        vertices, indices = torch.as_tensor(vertices).float(), torch.as_tensor(indices).long()
        if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= vertices.shape[0]):
            raise ValueError(f"tet indices outside [0, {vertices.shape[0]})")
        self.register_buffer("_grid_vertices", vertices, persistent=False)
        self.register_buffer("indices", indices, persistent=False)
        self._tables = None

    def normalize_grid_deformation(self, grid_vertex_offsets: torch.Tensor) -> torch.Tensor:
        return (self.points_range[1] - self.points_range[0]) / self.resolution * torch.tanh(grid_vertex_offsets)

    @property
    def grid_vertices(self) -> torch.Tensor:
        return self._grid_vertices

    def _edge_tables(self):
        """(edges int64, edges int32, tet_verts int32, tet_edges int32) on the device of `indices`, built once"""
        if self._tables is None or self._tables[0].device != self.indices.device:
            edges, tet_edges = tet_edge_tables(self.indices)
            self._tables = (edges, edges.int().contiguous(), self.indices.int().contiguous(), tet_edges.int().contiguous())
        return self._tables

    @property
    def all_edges(self) -> torch.Tensor:
        return self._edge_tables()[0]

    def forward(self, level: torch.Tensor, deformation: Optional[torch.Tensor] = None) -> Mesh:
        grid_vertices = self.grid_vertices
        if deformation is not None:
            grid_vertices = grid_vertices + self.normalize_grid_deformation(deformation)
        all_edges, edges, tet_verts, tet_edges = self._edge_tables()
        with torch.no_grad():
            v_pos, t_pos_idx = ops.marching_tetrahedra(level.detach().reshape(-1).to(grid_vertices.device), 0, verts=grid_vertices.detach(),
                                                       edges=edges, tet_verts=tet_verts, tet_edges=tet_edges)
        return Mesh(v_pos=v_pos, t_pos_idx=t_pos_idx, grid_vertices=grid_vertices, tet_edges=all_edges, grid_level=level,
                    grid_deformation=deformation)


class MarchingTetrahedraGridHelper(IsosurfaceHelper):
    """Kuhn form: the regular grid linspace(0,1,res)^3, six tetrahedra per cell, nothing but `resolution` stored"""

    def __init__(self, resolution: int) -> None:
        super().__init__()
        self.resolution = resolution
        self._grid_vertices: Optional[torch.Tensor] = None
        self.register_buffer("_dummy", torch.zeros(0, dtype=torch.float32), persistent=False)

    @property
    def grid_vertices(self) -> torch.Tensor:
        if self._grid_vertices is None or self._grid_vertices.device != self._dummy.device:
            self._grid_vertices = regular_grid_vertices(self.resolution, self._dummy.device)
        return self._grid_vertices

    def forward(self, level: torch.Tensor, deformation: Optional[torch.Tensor] = None) -> Mesh:
        if deformation is not None:
            warn(f"{self.__class__.__name__} does not support deformation. Ignoring.")
        dev = self._dummy.device
        with torch.no_grad():
            v_pos, t_pos_idx = ops.marching_tetrahedra(level.detach().reshape(-1).to(dev), self.resolution,
                                                       axis=torch.linspace(0, 1, self.resolution, device=dev))
        return Mesh(v_pos=v_pos, t_pos_idx=t_pos_idx, grid_vertices=self.grid_vertices, grid_level=level)
