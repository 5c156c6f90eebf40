"""Helpers of the mesh tests: canonical form, edge statistics, the Kuhn grid fields, an OBJ reader."""
import numpy as np


def canonical(verts, faces):
    """vertices sorted lexicographically by coordinate (stable: coincident vertices keep their order), faces re-indexed, each ROTATED (not
    reflected) to start at its smallest index, then sorted: winding stays significant, vertex and face order do not"""
    verts, faces = np.asarray(verts), np.asarray(faces).astype(np.int64).reshape(-1, 3)
    order = np.lexsort((verts[:, 2], verts[:, 1], verts[:, 0])) if len(verts) else np.zeros(0, np.int64)
    inv = np.empty(len(verts), np.int64)
    inv[order] = np.arange(len(verts))
    return verts[order], canonical_faces(inv[faces])


def canonical_faces(faces):
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return faces
    k = faces.argmin(axis=1)
    f = np.take_along_axis(faces, (k[:, None] + np.arange(3)[None]) % 3, axis=1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def edge_stats(faces):
    """(directed edges that occur more than once, undirected edges NOT in exactly two faces, number of undirected edges)"""
    f = np.asarray(faces).astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, dc = np.unique(d, axis=0, return_counts=True)
    _, uc = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return int((dc != 1).sum()), int((uc != 2).sum()), len(uc)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def read_obj(path):
    v, vn, f = [], [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:]])
            elif p[0] == "vn":
                vn.append([float(x) for x in p[1:]])
            elif p[0] == "f":
                f.append([[int(x) if x else 0 for x in c.split("/")] for c in p[1:]])
    return np.asarray(v), np.asarray(vn), np.asarray(f, np.int64)
