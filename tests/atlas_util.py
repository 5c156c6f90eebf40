"""Helpers of the atlas tests: the layout of csrc/atlas.hip restated in plain Python and float64 numpy, closest points on a triangle, the
texels of a bilinear lookup, readers for the OBJ (with `vt`) and the MTL."""
import math

import numpy as np

MAX_T = 8192


def layout_ref(F, T, g):
    """(n, c, L) of F faces in a T x T texture with gutter g, None when it must be refused (L < 1); no faces: no cells"""
    if F == 0:
        return (0, 0, 0)
    P = -(-F // 2)
    n = math.isqrt(P - 1) + 1           # ceil(sqrt(P)) in integers
    c = T // n
    L = c - 3 * g - 1
    return (n, c, L) if L >= 1 else None


def smallest_texture_size(F, g):
    """c >= 3 g + 2 <=> T >= n (3 g + 2)"""
    return 1 if F == 0 else (math.isqrt(-(-F // 2) - 1) + 1) * (3 * g + 2)


def smallest_pow2_texture_size(F, g):
    T = 1
    while T < smallest_texture_size(F, g):
        T *= 2
    return T


def corners_ref(F, T, g):
    """integer texel coordinates [3F, 2] of every face's three texture vertices, corner 0 1 2"""
    n, c, L = layout_ref(F, T, g)
    out = np.zeros((3 * F, 2), np.int64)
    for f in range(F):
        k = f // 2
        ox, oy = (k % n) * c, (k // n) * c
        if f % 2 == 0:
            tri = [(g, g), (g + L, g), (g, g + L)]
        else:
            tri = [(c - g, c - g), (c - g - L, c - g), (c - g, c - g - L)]
        out[3 * f:3 * f + 3] = [(ox + x, oy + y) for x, y in tri]
    return out


def ownership_ref(F, T, g):
    """face_id [T, T] (row j, column i; -1 = nobody) from the ownership rule alone"""
    n, c, L = layout_ref(F, T, g)
    fid = np.full((T, T), -1, np.int32)
    if F == 0:
        return fid
    j, i = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    ci, cj = i // c, j // c
    d = i % c + j % c + 1
    f = 2 * (cj * n + ci) + (d > c)
    own = (ci < n) & (cj < n) & (d != c) & (f < F)
    fid[own] = f[own]
    return fid


def closest_on_triangle(p, tri):
    """float64: p [N, 2], tri [N, 3, 2] -> (closest point of the closed triangle [N, 2], inside [N] bool).  Generic: the point itself where
    all three edge functions have the sign of the triangle's orientation (zero included), else the nearest of the three clamped edge projections."""
    p, tri = np.asarray(p, np.float64), np.asarray(tri, np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    cross = lambda u, v: u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    orient = np.sign(cross(b - a, c - a))
    inside = np.ones(len(p), bool)
    best, best_d = p.copy(), np.full(len(p), np.inf)
    for s, e in ((a, b), (b, c), (c, a)):
        inside &= cross(e - s, p - s) * orient >= 0
        t = np.clip(((p - s) * (e - s)).sum(1) / ((e - s) * (e - s)).sum(1), 0.0, 1.0)
        q = s + t[:, None] * (e - s)
        d = ((p - q) ** 2).sum(1)
        take = d < best_d
        best[take], best_d[take] = q[take], d[take]
    best[inside] = p[inside]
    return best, inside


def barycentric(q, tri):
    """float64 weights [N, 3] of q [N, 2] in tri [N, 3, 2]"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    den = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    w1 = ((q[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (q[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])) / den
    w2 = ((b[:, 0] - a[:, 0]) * (q[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (q[:, 0] - a[:, 0])) / den
    return np.stack([1.0 - w1 - w2, w1, w2], axis=1)


def bilinear_texels(x, y, T):
    """the four texels (j [N,4], i [N,4]) a bilinear lookup without mip-maps reads at continuous texel coordinates (x, y), clamped to the edge"""
    i0, j0 = np.floor(x - 0.5).astype(np.int64), np.floor(y - 0.5).astype(np.int64)
    i = np.stack([i0, i0 + 1, i0, i0 + 1], axis=1)
    j = np.stack([j0, j0, j0 + 1, j0 + 1], axis=1)
    return np.clip(j, 0, T - 1), np.clip(i, 0, T - 1)


def read_obj_uv(path):
    """-> (header lines before the first `v`, v, vn, vt, f [Nf,3,3] with 0 for an empty slot)"""
    header, v, vn, vt, f = [], [], [], [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:]])
            elif p[0] == "vn":
                vn.append([float(x) for x in p[1:]])
            elif p[0] == "vt":
                vt.append([float(x) for x in p[1:]])
            elif p[0] == "f":
                f.append([[int(x) if x else 0 for x in c.split("/")] for c in p[1:]])
            elif not v:
                header.append(line.rstrip("\n"))
    return header, np.asarray(v), np.asarray(vn), np.asarray(vt).reshape(-1, 2), np.asarray(f, np.int64).reshape(-1, 3, 3)
