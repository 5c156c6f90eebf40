"""Golden marching-tetrahedra meshes from the REFERENCE's own MarchingTetrahedraHelper._forward (threestudio/models/isosurface.py:168-227),
run on the CPU (build container only) over the Kuhn grid at res = 6 (216 vertices, 750 tets) given as explicit arrays, and four level
fields: a centred sphere (negative inside), two disjoint spheres, a torus, seeded Gaussian noise.  Only the grid arrays, the levels and
the reference's verts / faces are recorded.    python tests/golden/make_goldens_isosurface.py  ->  tests/golden/isosurface_mt_kuhn6.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

H.install()
for stub in ("threestudio.models.isosurface", "threestudio.models.mesh"):     # the harness stands in for these two; here the real ones are wanted
    sys.modules.pop(stub, None)

RES = 6


def fields(verts: torch.Tensor):
    c = torch.tensor([0.5, 0.5, 0.5])
    sphere = (verts - c).norm(dim=-1) - 0.3
    two = torch.minimum((verts - torch.tensor([0.25, 0.3, 0.3])).norm(dim=-1) - 0.18, (verts - torch.tensor([0.75, 0.7, 0.7])).norm(dim=-1) - 0.15)
    p = verts - c
    torus = torch.sqrt((torch.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.28) ** 2 + p[:, 2] ** 2) - 0.12
    noise = torch.randn(verts.shape[0], generator=torch.Generator().manual_seed(0))
    return {"sphere": sphere, "two_spheres": two, "torus": torus, "noise": noise}


if __name__ == "__main__":
    from scaledreamer_amd.isosurface import kuhn_grid_arrays
    from threestudio.models.isosurface import MarchingTetrahedraHelper

    verts, edges, tets, tet_edges = kuhn_grid_arrays(RES)
    real_load = np.load
    np.load = lambda path: {"vertices": verts.numpy(), "indices": tets.numpy()}     # the helper object without its file load
    try:
        helper = MarchingTetrahedraHelper(RES, "unused")
    finally:
        np.load = real_load
    out = dict(res=RES, verts=verts.numpy(), edges=edges.numpy().astype(np.int32), tet_verts=tets.numpy().astype(np.int32),
               tet_edges=tet_edges.numpy().astype(np.int32))
    for name, level in fields(verts).items():
        level = level.float().contiguous()
        v, f = helper._forward(verts, level.clone(), tets)
        out[f"{name}.level"] = level.numpy()
        out[f"{name}.verts"] = v.numpy()
        out[f"{name}.faces"] = f.numpy().astype(np.int32)
        print(name, tuple(v.shape), tuple(f.shape))
    np.savez_compressed(os.path.join(HERE, "isosurface_mt_kuhn6.npz"), **out)
    print("isosurface goldens written")
