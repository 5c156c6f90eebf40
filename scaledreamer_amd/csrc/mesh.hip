// mesh.hip — mesh extraction for gfx950: marching tetrahedra over a tetrahedral grid, connected components and compaction of the result
// (threestudio/models/isosurface.py:168-227 MarchingTetrahedraHelper._forward, threestudio/models/mesh.py:31-94 Mesh.remove_outlier).
// The grid comes in one of two forms:
//   explicit   verts[Nv,3], edges[Ne,2] (unique, a < b, sorted), tet_verts[Nt,4], tet_edges[Nt,6] (edges 01 02 03 12 13 23 of every tet)
//   Kuhn       res only: vertices linspace(0,1,res)^3 in `ij` order (z fastest), every cell split into the six tetrahedra around its main
//              diagonal; vertex v owns the seven edge slots 7 v + d - 1, d = (di dj dk) in 1..7 the offset of the far end, and cell c the
//              six tet slots 6 c + t.  Slots of edges that would leave the grid exist and never cross.  Nothing is materialised.
// Passes (asd_mt_count, then asd_mt_emit once the host has read the two totals and allocated the outputs):
//   1  crossing flag per edge slot (exactly one end has level > 0) and triangle count per tet slot (16-case table)
//   2  exclusive scan of both arrays, in place (asd_scan_i32_blocks: tile sums, one block over the tile sums, tiles again)
//   3  one vertex per crossing edge at its scanned slot: w_a = -s_b / (s_a - s_b), w_b = s_a / (s_a - s_b), v = p_a w_a + p_b w_b — the
//      reference's three operations, IEEE division, no contraction (the library is built with -ffp-contract=off)
//   4  the faces of every tet at its scanned slot, their corners looked up through the edge slots' scanned offsets
// No atomics: slot order is edge order and tet order, so two runs give the same bits and the vertices come out in the order of the
// reference's torch.unique over the crossing edges.  Roofline: bandwidth-trivial (res 128: 2.1 M levels, 14.7 M + 12.3 M int32 slots, each
// written once, scanned once and read once: ~0.5 GB of traffic per extraction); neighbouring threads take neighbouring z, so the level
// loads of the Kuhn passes are coalesced and the seven neighbours of a vertex are its cell's corners.
// Components: min-label hooking over the faces + pointer jumping; a round reports on the device whether it changed anything.
#include "asd_common.h"

// ---- the 16 cases ------------------------------------------------------------------------------------------------------------------
// Case index: bit v set iff level[tet vertex v] > 0.  Local edge ids: 01 02 03 12 13 23 -> 0..5.  The table is DERIVED, by these rules:
//   one vertex v on its own side (cases with one or three bits): one triangle on the three edges (v,a), (v,b), (v,c), with (a,b,c) ordered
//     so that the permutation (v,a,b,c) of (0,1,2,3) is ODD when v is the positive vertex and EVEN when it is the negative one.  On a tet
//     with det[v1-v0, v2-v0, v3-v0] > 0 that is the winding whose normal points to the positive side.
//   two and two (p < q positive): the quad is the triangle of p alone with the edge (p,q) cut off by q coming over to p's side: in the
//     rotation (a,q,c) of that triangle the quad runs (p,a) (q,a) (q,c) (p,c) — same winding.  Its diagonal joins a pair of OPPOSITE tet
//     edges; of the two pairs that cross, 02|13 is taken when it is one of them, else 03|12.
// tests/golden/isosurface_mt_kuhn6.npz pins the result against the reference's own faces.
static constexpr int mt_edge_id(int a, int b) { return (a < b ? a : b) == 0 ? (a < b ? b : a) - 1 : a + b; }
static constexpr bool mt_odd(int a, int b, int c, int d) {
    const int p[4] = {a, b, c, d};
    int inv = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) inv += p[i] > p[j];
    return inv & 1;
}
// the triangle of lone vertex v as the far ends (a,b,c) of its three edges
static constexpr void mt_lone(int v, bool positive, int (&o)[3]) {
    int n = 0;
    for (int u = 0; u < 4; ++u)
        if (u != v) o[n++] = u;
    if (mt_odd(v, o[0], o[1], o[2]) != positive) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
}
// bits 0..17: six local edge ids, three bits each (two triangles at most); bits 18..19: the number of triangles
static constexpr uint32_t mt_case(int occ) {
    int pos[4] = {0, 0, 0, 0}, neg[4] = {0, 0, 0, 0}, np = 0, nn = 0;
    for (int v = 0; v < 4; ++v) {
        if ((occ >> v) & 1) pos[np++] = v; else neg[nn++] = v;
    }
    int e[6] = {0, 0, 0, 0, 0, 0}, n = 0;
    if (np == 1 || np == 3) {
        const int v = np == 1 ? pos[0] : neg[0];
        int o[3] = {0, 0, 0};
        mt_lone(v, np == 1, o);
        for (int k = 0; k < 3; ++k) e[k] = mt_edge_id(v, o[k]);
        n = 1;
    } else if (np == 2) {
        const int p = pos[0], q = pos[1];
        int o[3] = {0, 0, 0};
        mt_lone(p, true, o);
        while (o[1] != q) { const int t = o[0]; o[0] = o[1]; o[1] = o[2]; o[2] = t; }
        const int c[4] = {mt_edge_id(p, o[0]), mt_edge_id(q, o[0]), mt_edge_id(q, o[2]), mt_edge_id(p, o[2])};
        const bool d02 = c[0] + c[2] == 5 && (c[0] == 1 || c[0] == 4);      // the diagonal c0-c2 is the pair 02|13
        const bool d13 = c[1] + c[3] == 5 && (c[1] == 1 || c[1] == 4);      // the diagonal c1-c3 is
        const bool first = d02 || (!d13 && (c[0] == 2 || c[0] == 3));       // else whichever diagonal is 03|12
        if (first) { e[0] = c[0]; e[1] = c[1]; e[2] = c[2]; e[3] = c[0]; e[4] = c[2]; e[5] = c[3]; }
        else { e[0] = c[1]; e[1] = c[2]; e[2] = c[3]; e[3] = c[1]; e[4] = c[3]; e[5] = c[0]; }
        n = 2;
    }
    uint32_t w = (uint32_t)n << 18;
    for (int k = 0; k < 6; ++k) w |= (uint32_t)e[k] << (3 * k);
    return w;
}
#define MT_ALL_CASES { mt_case(0), mt_case(1), mt_case(2), mt_case(3), mt_case(4), mt_case(5), mt_case(6), mt_case(7), mt_case(8), mt_case(9), \
                       mt_case(10), mt_case(11), mt_case(12), mt_case(13), mt_case(14), mt_case(15) }
static const uint32_t mt_table_host[16] = MT_ALL_CASES;
__constant__ const uint32_t mt_table[16] = MT_ALL_CASES;
__device__ __forceinline__ int mt_ntri(uint32_t w) { return (int)(w >> 18); }
__device__ __forceinline__ int mt_corner(uint32_t w, int q) { return (int)((w >> (3 * q)) & 7u); }
// the two ends of local edge l
__constant__ const unsigned char mt_edge_lo[6] = {0, 0, 0, 1, 1, 2};
__constant__ const unsigned char mt_edge_hi[6] = {1, 2, 3, 2, 3, 3};

// ---- the Kuhn grid -----------------------------------------------------------------------------------------------------------------
// Corner codes are (di dj dk) as three bits.  Tet t of a cell walks the axes in the t-th permutation, cell corner 0 -> 7; the odd
// permutations have their two middle vertices exchanged, so all six have det > 0 and neighbouring tets wind their triangles alike.
//   (i,j,k) 0 4 6 7   (i,k,j) 0 5 4 7   (j,i,k) 0 6 2 7   (j,k,i) 0 2 3 7   (k,i,j) 0 1 5 7   (k,j,i) 0 3 1 7
// scaledreamer_amd/isosurface.py:kuhn_grid_arrays builds the same grid as explicit arrays from this list.
__constant__ const unsigned char kuhn_tet[6][4] = {{0, 4, 6, 7}, {0, 5, 4, 7}, {0, 6, 2, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 3, 1, 7}};
#define MT_MAX_RES 512       // 7 * 512^3 edge slots stay below 2^31
__device__ __forceinline__ int64_t kuhn_voff(int code, int res) {
    return (int64_t)((code >> 2) & 1) * res * res + (int64_t)((code >> 1) & 1) * res + (code & 1);
}
// edge slot of the tet edge between corner codes x and y of the cell whose corner 0 is vertex vc: any two corners of a Kuhn tet are nested
// bit sets, the smaller code is the edge's first (lower-numbered) vertex and the difference its direction
__device__ __forceinline__ int64_t kuhn_edge_slot(int64_t vc, int x, int y, int res) {
    const int lo = x < y ? x : y, d = x ^ y;
    return 7 * (vc + kuhn_voff(lo, res)) + d - 1;
}

// pass 1, Kuhn: one thread per grid vertex (z fastest).  The seven far ends of its edges are the other corners of the cell it is corner 0
// of, so the same eight levels give the cell's six triangle counts.
__global__ __launch_bounds__(256) void mt_kuhn_count_kernel(const float* __restrict__ level, int res, int32_t* __restrict__ edge_cnt,
                                                            int32_t* __restrict__ tet_cnt) {
    const int64_t nv = (int64_t)res * res * res;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
        const int k = (int)(v % res), j = (int)((v / res) % res), i = (int)(v / ((int64_t)res * res));
        bool occ[8];
        occ[0] = level[v] > 0.f;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            const bool in = i + ((d >> 2) & 1) < res && j + ((d >> 1) & 1) < res && k + (d & 1) < res;
            occ[d] = in ? level[v + kuhn_voff(d, res)] > 0.f : occ[0];      // outside the grid: never a crossing
            edge_cnt[7 * v + d - 1] = occ[d] != occ[0];
        }
        if (i < res - 1 && j < res - 1 && k < res - 1) {
            const int64_t c = ((int64_t)i * (res - 1) + j) * (res - 1) + k;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int cs = (int)occ[kuhn_tet[t][0]] | (int)occ[kuhn_tet[t][1]] << 1 | (int)occ[kuhn_tet[t][2]] << 2 | (int)occ[kuhn_tet[t][3]] << 3;
                tet_cnt[6 * c + t] = mt_ntri(mt_table[cs]);
            }
        }
    }
}

// the reference's interpolation, operation for operation
__device__ __forceinline__ void mt_interp(float sa, float sb, const float (&pa)[3], const float (&pb)[3], float* __restrict__ out) {
    const float nsb = -sb;
    const float den = sa + nsb;
    const float wa = nsb / den, wb = sa / den;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = pa[c] * wa + pb[c] * wb;
}

// pass 3, Kuhn: one thread per grid vertex, its crossing edges
__global__ __launch_bounds__(256) void mt_kuhn_verts_kernel(const float* __restrict__ level, const float* __restrict__ axis, int res,
                                                            const int32_t* __restrict__ edge_off, int64_t n_out, float* __restrict__ out) {
    const int64_t nv = (int64_t)res * res * res;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
        const int k = (int)(v % res), j = (int)((v / res) % res), i = (int)(v / ((int64_t)res * res));
        const float sa = level[v];
        const float pa[3] = {axis[i], axis[j], axis[k]};
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            const int di = (d >> 2) & 1, dj = (d >> 1) & 1, dk = d & 1;
            if (i + di >= res || j + dj >= res || k + dk >= res) continue;
            const float sb = level[v + kuhn_voff(d, res)];
            if ((sa > 0.f) == (sb > 0.f)) continue;
            const int64_t slot = edge_off[7 * v + d - 1];
            if (slot < 0 || slot >= n_out) continue;
            const float pb[3] = {axis[i + di], axis[j + dj], axis[k + dk]};
            mt_interp(sa, sb, pa, pb, out + 3 * slot);
        }
    }
}

// pass 4, Kuhn: one thread per cell, the triangles of its six tets
__global__ __launch_bounds__(256) void mt_kuhn_faces_kernel(const float* __restrict__ level, int res, const int32_t* __restrict__ edge_off,
                                                            const int32_t* __restrict__ tet_off, int64_t n_out, int64_t* __restrict__ faces) {
    const int rc = res - 1;
    const int64_t nc = (int64_t)rc * rc * rc;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nc; c += (int64_t)gridDim.x * 256) {
        const int k = (int)(c % rc), j = (int)((c / rc) % rc), i = (int)(c / ((int64_t)rc * rc));
        const int64_t vc = ((int64_t)i * res + j) * res + k;
        bool occ[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) occ[d] = level[vc + kuhn_voff(d, res)] > 0.f;
        bool all = true, none = true;
#pragma unroll
        for (int d = 0; d < 8; ++d) { all = all && occ[d]; none = none && !occ[d]; }
        if (all || none) continue;
        for (int t = 0; t < 6; ++t) {
            const unsigned char* o = kuhn_tet[t];
            const int cs = (int)occ[o[0]] | (int)occ[o[1]] << 1 | (int)occ[o[2]] << 2 | (int)occ[o[3]] << 3;
            const uint32_t w = mt_table[cs];
            const int n = mt_ntri(w);
            if (n == 0) continue;
            const int64_t base = tet_off[6 * c + t];
            if (base < 0 || base + n > n_out) continue;
            for (int q = 0; q < 3 * n; ++q) {
                const int l = mt_corner(w, q);
                faces[3 * base + q] = edge_off[kuhn_edge_slot(vc, o[mt_edge_lo[l]], o[mt_edge_hi[l]], res)];
            }
        }
    }
}

// ---- the explicit grid -------------------------------------------------------------------------------------------------------------
// An index outside its table makes the edge or the tet count as empty: nothing is read or written through it.
__global__ __launch_bounds__(256) void mt_edge_count_kernel(const float* __restrict__ level, int64_t n_grid, const int32_t* __restrict__ edges,
                                                            int64_t n_edges, int32_t* __restrict__ edge_cnt) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * 256) {
        const int64_t a = edges[2 * e], b = edges[2 * e + 1];
        const bool ok = a >= 0 && a < n_grid && b >= 0 && b < n_grid;
        edge_cnt[e] = ok && ((level[a] > 0.f) != (level[b] > 0.f));
    }
}

__device__ __forceinline__ int mt_tet_case(const float* __restrict__ level, int64_t n_grid, const int32_t* __restrict__ tv) {
    int cs = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t v = tv[u];
        if (v < 0 || v >= n_grid) return 0;
        cs |= (int)(level[v] > 0.f) << u;
    }
    return cs;
}

__global__ __launch_bounds__(256) void mt_tet_count_kernel(const float* __restrict__ level, int64_t n_grid, const int32_t* __restrict__ tet_verts,
                                                           int64_t n_tets, int32_t* __restrict__ tet_cnt) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_tets; t += (int64_t)gridDim.x * 256)
        tet_cnt[t] = mt_ntri(mt_table[mt_tet_case(level, n_grid, tet_verts + 4 * t)]);
}

__global__ __launch_bounds__(256) void mt_edge_verts_kernel(const float* __restrict__ level, const float* __restrict__ verts, int64_t n_grid,
                                                            const int32_t* __restrict__ edges, int64_t n_edges,
                                                            const int32_t* __restrict__ edge_off, int64_t n_out, float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * 256) {
        const int64_t a = edges[2 * e], b = edges[2 * e + 1];
        if (a < 0 || a >= n_grid || b < 0 || b >= n_grid) continue;
        const float sa = level[a], sb = level[b];
        if ((sa > 0.f) == (sb > 0.f)) continue;
        const int64_t slot = edge_off[e];
        if (slot < 0 || slot >= n_out) continue;
        const float pa[3] = {verts[3 * a], verts[3 * a + 1], verts[3 * a + 2]};
        const float pb[3] = {verts[3 * b], verts[3 * b + 1], verts[3 * b + 2]};
        mt_interp(sa, sb, pa, pb, out + 3 * slot);
    }
}

__global__ __launch_bounds__(256) void mt_tet_faces_kernel(const float* __restrict__ level, int64_t n_grid, const int32_t* __restrict__ tet_verts,
                                                           const int32_t* __restrict__ tet_edges, int64_t n_tets, int64_t n_edges,
                                                           const int32_t* __restrict__ edge_off, const int32_t* __restrict__ tet_off,
                                                           int64_t n_out, int64_t* __restrict__ faces) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_tets; t += (int64_t)gridDim.x * 256) {
        const uint32_t w = mt_table[mt_tet_case(level, n_grid, tet_verts + 4 * t)];
        const int n = mt_ntri(w);
        if (n == 0) continue;
        const int64_t base = tet_off[t];
        if (base < 0 || base + n > n_out) continue;
        for (int q = 0; q < 3 * n; ++q) {
            const int64_t e = tet_edges[6 * t + mt_corner(w, q)];
            faces[3 * base + q] = e >= 0 && e < n_edges ? edge_off[e] : 0;
        }
    }
}

// ---- exclusive scan over many blocks -----------------------------------------------------------------------------------------------
// A tile is SCAN_TILE consecutive entries: 256 threads x 8, two int4 per thread.  (1) tile sums, (2) one block scans the tile sums in
// place, (3) every tile again: thread-local prefix, wave prefix (ballot-free: the counts are not 0/1 in general), the four wave totals
// through LDS, plus the tile's base.  In place: a thread writes only the eight entries it has read itself.
#define SCAN_THREADS 256
#define SCAN_PER_THREAD 8
#define SCAN_TILE (SCAN_THREADS * SCAN_PER_THREAD)

__device__ __forceinline__ int scan_wave_incl(int v) {
    const int lane = asd_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ void scan_load8(const int32_t* __restrict__ x, int64_t at, int64_t n, int (&v)[SCAN_PER_THREAD]) {
    if (at + SCAN_PER_THREAD <= n) {        // `x` is 16-byte aligned and `at` a multiple of 8
        const int4 a = *reinterpret_cast<const int4*>(x + at), b = *reinterpret_cast<const int4*>(x + at + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int q = 0; q < SCAN_PER_THREAD; ++q) v[q] = at + q < n ? x[at + q] : 0;
    }
}

// sum over the block, valid in every thread
__device__ __forceinline__ int scan_block_sum(int v, int* __restrict__ lds) {
    const int incl = scan_wave_incl(v);
    if (asd_lane() == 63) lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_sums_kernel(const int32_t* __restrict__ x, int64_t n, int32_t* __restrict__ sums) {
    __shared__ int lds[SCAN_THREADS / 64];
    int v[SCAN_PER_THREAD];
    scan_load8(x, (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER_THREAD, n, v);
    int s = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) s += v[q];
    s = scan_block_sum(s, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// one block: sums[0..m) -> their exclusive scan in place, the grand total to total[0]
__global__ __launch_bounds__(1024) void scan_sums_kernel(int32_t* __restrict__ sums, int m, int32_t* __restrict__ total) {
    __shared__ int lds[16];
    __shared__ int carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < m; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int v = i < m ? sums[i] : 0;
        const int incl = scan_wave_incl(v);
        if (asd_lane() == 63) lds[threadIdx.x >> 6] = incl;
        __syncthreads();
        int before = carry_s, all = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < (int)(threadIdx.x >> 6)) before += lds[w];
            all += lds[w];
        }
        if (i < m) sums[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry_s;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_tiles_kernel(const int32_t* x, int64_t n, const int32_t* __restrict__ sums, int32_t* out) {
    __shared__ int lds[SCAN_THREADS / 64];
    const int64_t at = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    int v[SCAN_PER_THREAD];
    scan_load8(x, at, n, v);
    int s = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) s += v[q];
    const int incl = scan_wave_incl(s);
    if (asd_lane() == 63) lds[threadIdx.x >> 6] = incl;
    __syncthreads();
    int run = sums[blockIdx.x] + incl - s;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) run += lds[w];
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; ++q) {
        if (at + q < n) out[at + q] = run;
        run += v[q];
    }
}

static int64_t scan_blocks_ints(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

static int scan_blocks_launch(const int32_t* count, int64_t n, int32_t* offset, int32_t* total, int32_t* sums, hipStream_t s) {
    const int tiles = (int)scan_blocks_ints(n);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(tiles), dim3(SCAN_THREADS), 0, s, count, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, s, sums, tiles, total);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(tiles), dim3(SCAN_THREADS), 0, s, count, n, (const int32_t*)sums, offset);
    return tiles;
}

// ---- connected components, compaction ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_init_kernel(int32_t* __restrict__ label, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) label[v] = (int32_t)v;
}

// label[v] <= v always, and a label only ever decreases: the chain label[label[...]] ends in a root r = label[r]
__global__ __launch_bounds__(256) void cc_hook_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_verts, int32_t* label,
                                                      int32_t* __restrict__ changed) {
    bool any = false;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * 256) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a < 0 || a >= n_verts || b < 0 || b >= n_verts || c < 0 || c >= n_verts) continue;
        const int la = label[a], lb = label[b], lc = label[c];
        const int m = min(la, min(lb, lc));
        if (la != m) { atomicMin(label + la, m); atomicMin(label + a, m); any = true; }
        if (lb != m) { atomicMin(label + lb, m); atomicMin(label + b, m); any = true; }
        if (lc != m) { atomicMin(label + lc, m); atomicMin(label + c, m); any = true; }
    }
    if (__ballot(any) != 0ull && asd_lane() == 0) changed[0] = 1;      // one plain store of the same value per wave that saw a change
}

__global__ __launch_bounds__(256) void cc_jump_kernel(int32_t* label, int64_t n_verts) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_verts; v += (int64_t)gridDim.x * 256) {
        int l = label[v];
        for (int hop = 0; hop < 1 << 30; ++hop) {       // roots do not move during this kernel: the walk ends at one
            const int up = label[l];
            if (up == l) break;
            l = up;
        }
        label[v] = l;
    }
}

__global__ __launch_bounds__(256) void cc_face_count_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_verts,
                                                            const int32_t* __restrict__ label, int32_t* __restrict__ count) {
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * 256) {
        const int64_t a = faces[3 * f];
        if (a >= 0 && a < n_verts) atomicAdd(count + label[a], 1);       // integer adds: any order, one result
    }
}

__global__ __launch_bounds__(256) void cc_keep_kernel(const int64_t* __restrict__ faces, int64_t n_faces, int64_t n_verts,
                                                      const int32_t* __restrict__ label, const int32_t* __restrict__ count, int threshold,
                                                      int32_t* __restrict__ v_keep, int32_t* __restrict__ f_keep) {
    const int64_t n = n_verts > n_faces ? n_verts : n_faces;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (i < n_verts) v_keep[i] = count[label[i]] >= threshold;
        if (i < n_faces) {
            const int64_t a = faces[3 * i];
            f_keep[i] = a >= 0 && a < n_verts && count[label[a]] >= threshold;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_compact_kernel(const float* __restrict__ v_pos, const int64_t* __restrict__ faces, int64_t n_verts,
                                                           int64_t n_faces, const int32_t* __restrict__ v_keep, const int32_t* __restrict__ v_map,
                                                           const int32_t* __restrict__ f_keep, const int32_t* __restrict__ f_map,
                                                           int64_t n_verts_out, int64_t n_faces_out, float* __restrict__ v_out,
                                                           int64_t* __restrict__ f_out) {
    const int64_t n = n_verts > n_faces ? n_verts : n_faces;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (i < n_verts && v_keep[i]) {
            const int64_t o = v_map[i];
            if (o >= 0 && o < n_verts_out) { v_out[3 * o] = v_pos[3 * i]; v_out[3 * o + 1] = v_pos[3 * i + 1]; v_out[3 * o + 2] = v_pos[3 * i + 2]; }
        }
        if (i < n_faces && f_keep[i]) {
            const int64_t o = f_map[i];
            if (o < 0 || o >= n_faces_out) continue;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int64_t v = faces[3 * i + q];
                f_out[3 * o + q] = v >= 0 && v < n_verts ? v_map[v] : 0;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// The workspace of asd_mt_count / asd_mt_emit in int32 from its start: asd_mt_workspace returns `total`, the passes take every pointer from here.
static asd_mt_layout mt_layout_init(int32_t res, int64_t n_edges, int64_t n_tets) {
    asd_mt_layout L;
    asd_ws_cursor w;
    L.n_edge_slots = res > 0 ? 7 * (int64_t)res * res * res : n_edges;
    L.n_tet_slots = res > 0 ? 6 * (int64_t)(res - 1) * (res - 1) * (res - 1) : n_tets;
    L.edge_off = w.take(L.n_edge_slots);
    L.tet_off = w.take(L.n_tet_slots);
    L.scan = w.take(scan_blocks_ints(L.n_edge_slots > L.n_tet_slots ? L.n_edge_slots : L.n_tet_slots));
    L.counts = w.take(2);
    L.total = w.o;
    return L;
}

static bool mt_grid_ok(const char* fn, int32_t res, int64_t n_grid, int64_t n_edges, int64_t n_tets) {
    if (res != 0 && (res < 2 || res > MT_MAX_RES)) {
        asd_set_error("%s: res must be 0 (explicit grid) or in [2, %d] (got %d)", fn, MT_MAX_RES, res);
        return false;
    }
    if (res == 0 && (n_grid < 0 || n_edges < 0 || n_tets < 0 || n_grid > INT32_MAX || n_edges > INT32_MAX || n_tets > INT32_MAX / 2)) {
        asd_set_error("%s: grid sizes must not be negative and must index with 32 bits", fn);
        return false;
    }
    return true;
}

extern "C" {

int asd_mt_case_table(int32_t* table) {
    ASD_CHECK_ARG(table, "null argument");
    for (int c = 0; c < 16; ++c) {
        table[7 * c] = (int32_t)(mt_table_host[c] >> 18);
        for (int q = 0; q < 6; ++q) table[7 * c + 1 + q] = q < 3 * table[7 * c] ? (int32_t)((mt_table_host[c] >> (3 * q)) & 7u) : -1;
    }
    return ASD_OK;
}

int asd_scan_i32_blocks_workspace(int64_t n, int64_t* n_ints) {
    ASD_CHECK_ARG(n_ints, "null argument");
    ASD_CHECK_ARG(n >= 0 && n <= INT32_MAX, "n must be in [0, 2^31)");
    *n_ints = scan_blocks_ints(n);
    return ASD_OK;
}

int asd_scan_i32_blocks(const int32_t* count, int64_t n, int32_t* offset, int32_t* total, int32_t* workspace, void* stream) {
    ASD_CHECK_ARG(total, "null argument");
    ASD_CHECK_ARG(n >= 0 && n <= INT32_MAX, "n must be in [0, 2^31)");
    if (n == 0) {
        if (hipMemsetAsync(total, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
            asd_set_error("%s: hipMemsetAsync failed", __func__);
            return ASD_ERR_LAUNCH;
        }
        return ASD_OK;
    }
    ASD_CHECK_ARG(count && offset && workspace, "null argument");
    ASD_CHECK_ARG(((uintptr_t)count & 15) == 0, "count must be 16-byte aligned");
    scan_blocks_launch(count, n, offset, total, workspace, (hipStream_t)stream);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mt_workspace(int32_t res, int64_t n_edges, int64_t n_tets, asd_mt_layout* layout, int64_t* n_ints) {
    ASD_CHECK_ARG(layout || n_ints, "null argument");
    if (!mt_grid_ok(__func__, res, 0, n_edges, n_tets)) return ASD_ERR_ARG;
    const asd_mt_layout L = mt_layout_init(res, n_edges, n_tets);
    if (layout) *layout = L;
    if (n_ints) *n_ints = L.total;
    return ASD_OK;
}

int asd_mt_count(const float* level, int32_t res, int64_t n_grid, const int32_t* edges, int64_t n_edges, const int32_t* tet_verts, int64_t n_tets,
                 int32_t* workspace, void* stream) {
    ASD_CHECK_ARG(level && workspace, "null argument");
    ASD_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    if (!mt_grid_ok(__func__, res, n_grid, n_edges, n_tets)) return ASD_ERR_ARG;
    ASD_CHECK_ARG(res > 0 || ((edges || n_edges == 0) && (tet_verts || n_tets == 0)), "the explicit grid needs its edge and tet tables");
    hipStream_t s = (hipStream_t)stream;
    const asd_mt_layout L = mt_layout_init(res, n_edges, n_tets);
    int32_t *const edge_off = workspace + L.edge_off, *const tet_off = workspace + L.tet_off, *const sums = workspace + L.scan;
    int32_t* const counts = workspace + L.counts;
    if (res > 0) {
        hipLaunchKernelGGL(mt_kuhn_count_kernel, dim3(asd_grid_for((int64_t)res * res * res, 256)), dim3(256), 0, s, level, (int)res, edge_off, tet_off);
    } else {
        if (n_edges > 0)
            hipLaunchKernelGGL(mt_edge_count_kernel, dim3(asd_grid_for(n_edges, 256)), dim3(256), 0, s, level, n_grid, edges, n_edges, edge_off);
        if (n_tets > 0)
            hipLaunchKernelGGL(mt_tet_count_kernel, dim3(asd_grid_for(n_tets, 256)), dim3(256), 0, s, level, n_grid, tet_verts, n_tets, tet_off);
    }
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s) != hipSuccess) {
        asd_set_error("%s: hipMemsetAsync failed", __func__);
        return ASD_ERR_LAUNCH;
    }
    if (L.n_edge_slots > 0) scan_blocks_launch(edge_off, L.n_edge_slots, edge_off, counts, sums, s);
    if (L.n_tet_slots > 0) scan_blocks_launch(tet_off, L.n_tet_slots, tet_off, counts + 1, sums, s);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mt_emit(const float* level, int32_t res, const float* axis, const float* verts, int64_t n_grid, const int32_t* edges, int64_t n_edges,
                const int32_t* tet_verts, const int32_t* tet_edges, int64_t n_tets, const int32_t* workspace, int64_t n_verts_out,
                int64_t n_faces_out, float* out_verts, int64_t* out_faces, void* stream) {
    ASD_CHECK_ARG(level && workspace, "null argument");
    if (!mt_grid_ok(__func__, res, n_grid, n_edges, n_tets)) return ASD_ERR_ARG;
    ASD_CHECK_ARG(n_verts_out >= 0 && n_faces_out >= 0, "output sizes must not be negative");
    ASD_CHECK_ARG((out_verts || n_verts_out == 0) && (out_faces || n_faces_out == 0), "null output");
    ASD_CHECK_ARG(res == 0 || axis, "the Kuhn grid needs the res coordinates of its axis");
    ASD_CHECK_ARG(res > 0 || ((verts || n_grid == 0) && (edges || n_edges == 0) && ((tet_verts && tet_edges) || n_tets == 0)),
                  "the explicit grid needs its vertex, edge and tet tables");
    hipStream_t s = (hipStream_t)stream;
    const asd_mt_layout L = mt_layout_init(res, n_edges, n_tets);
    const int32_t *const edge_off = workspace + L.edge_off, *const tet_off = workspace + L.tet_off;
    if (res > 0) {
        if (n_verts_out > 0)
            hipLaunchKernelGGL(mt_kuhn_verts_kernel, dim3(asd_grid_for((int64_t)res * res * res, 256)), dim3(256), 0, s, level, axis, (int)res, edge_off,
                               n_verts_out, out_verts);
        if (n_faces_out > 0)
            hipLaunchKernelGGL(mt_kuhn_faces_kernel, dim3(asd_grid_for((int64_t)(res - 1) * (res - 1) * (res - 1), 256)), dim3(256), 0, s, level, (int)res,
                               edge_off, tet_off, n_faces_out, out_faces);
    } else {
        if (n_verts_out > 0 && n_edges > 0)
            hipLaunchKernelGGL(mt_edge_verts_kernel, dim3(asd_grid_for(n_edges, 256)), dim3(256), 0, s, level, verts, n_grid, edges, n_edges, edge_off,
                               n_verts_out, out_verts);
        if (n_faces_out > 0 && n_tets > 0)
            hipLaunchKernelGGL(mt_tet_faces_kernel, dim3(asd_grid_for(n_tets, 256)), dim3(256), 0, s, level, n_grid, tet_verts, tet_edges, n_tets, n_edges,
                               edge_off, tet_off, n_faces_out, out_faces);
    }
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mesh_cc_round(const int64_t* faces, int64_t n_faces, int64_t n_verts, int32_t first, int32_t* labels, int32_t* changed, void* stream) {
    ASD_CHECK_ARG(labels && changed && (faces || n_faces == 0), "null argument");
    ASD_CHECK_ARG(n_faces >= 0 && n_verts >= 0 && n_verts <= INT32_MAX && n_faces <= INT32_MAX, "sizes must be in [0, 2^31)");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(changed, 0, sizeof(int32_t), s) != hipSuccess) {
        asd_set_error("%s: hipMemsetAsync failed", __func__);
        return ASD_ERR_LAUNCH;
    }
    if (n_verts == 0) return ASD_OK;
    if (first) hipLaunchKernelGGL(cc_init_kernel, dim3(asd_grid_for(n_verts, 256)), dim3(256), 0, s, labels, n_verts);
    if (n_faces > 0) {
        hipLaunchKernelGGL(cc_hook_kernel, dim3(asd_grid_for(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_verts, labels, changed);
        hipLaunchKernelGGL(cc_jump_kernel, dim3(asd_grid_for(n_verts, 256)), dim3(256), 0, s, labels, n_verts);
    }
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mesh_face_counts(const int64_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* labels, int32_t* counts, void* stream) {
    ASD_CHECK_ARG((labels && counts) || n_verts == 0, "null argument");
    ASD_CHECK_ARG(faces || n_faces == 0, "null argument");
    ASD_CHECK_ARG(n_faces >= 0 && n_verts >= 0 && n_verts <= INT32_MAX && n_faces <= INT32_MAX, "sizes must be in [0, 2^31)");
    if (n_verts == 0) return ASD_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n_verts * sizeof(int32_t), s) != hipSuccess) {
        asd_set_error("%s: hipMemsetAsync failed", __func__);
        return ASD_ERR_LAUNCH;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(cc_face_count_kernel, dim3(asd_grid_for(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_verts, labels, counts);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mesh_keep(const int64_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* labels, const int32_t* counts, int32_t threshold,
                  int32_t* v_keep, int32_t* f_keep, void* stream) {
    ASD_CHECK_ARG((labels && counts && v_keep) || n_verts == 0, "null argument");
    ASD_CHECK_ARG((faces && f_keep) || n_faces == 0, "null argument");
    ASD_CHECK_ARG(n_faces >= 0 && n_verts >= 0 && n_verts <= INT32_MAX && n_faces <= INT32_MAX, "sizes must be in [0, 2^31)");
    if (n_verts == 0 && n_faces == 0) return ASD_OK;
    hipLaunchKernelGGL(cc_keep_kernel, dim3(asd_grid_for(n_verts > n_faces ? n_verts : n_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces,
                       n_verts, labels, counts, (int)threshold, v_keep, f_keep);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

int asd_mesh_compact(const float* v_pos, const int64_t* faces, int64_t n_verts, int64_t n_faces, const int32_t* v_keep, const int32_t* v_map,
                     const int32_t* f_keep, const int32_t* f_map, int64_t n_verts_out, int64_t n_faces_out, float* v_out, int64_t* f_out,
                     void* stream) {
    ASD_CHECK_ARG((v_pos && v_keep && v_map) || n_verts == 0, "null argument");
    ASD_CHECK_ARG((faces && f_keep && f_map) || n_faces == 0, "null argument");
    ASD_CHECK_ARG(n_faces >= 0 && n_verts >= 0 && n_verts <= INT32_MAX && n_faces <= INT32_MAX, "sizes must be in [0, 2^31)");
    ASD_CHECK_ARG(n_verts_out >= 0 && n_verts_out <= n_verts && n_faces_out >= 0 && n_faces_out <= n_faces, "output sizes must lie in [0, input size]");
    ASD_CHECK_ARG((v_out || n_verts_out == 0) && (f_out || n_faces_out == 0), "null output");
    if (n_verts == 0 && n_faces == 0) return ASD_OK;
    hipLaunchKernelGGL(mesh_compact_kernel, dim3(asd_grid_for(n_verts > n_faces ? n_verts : n_faces, 256)), dim3(256), 0, (hipStream_t)stream, v_pos,
                       faces, n_verts, n_faces, v_keep, v_map, f_keep, f_map, n_verts_out, n_faces_out, v_out, f_out);
    ASD_LAUNCH_CHECK();
    return ASD_OK;
}

}  // extern "C"
