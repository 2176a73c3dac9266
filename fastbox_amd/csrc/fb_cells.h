// Cell binning of a periodic particle set, shared by the friends-of-friends search (fb_fof.hip) and the pair counts
// (fb_pairs.hip): wrapping, minimum-image differences, the cell of a particle, the occupancy histogram, its exclusive scan,
// the permuted copy of the wrapped positions and the list of the further tiles of crowded cells.
//
// No contraction: the wrapped positions and the minimum-image differences must be the doubles of the numpy statements
// (tests/fof_numpy.py, tests/pairs_numpy.py).  The pragma below is at file scope on purpose: it switches contraction off for
// the rest of any source that includes this file, because the callers' own d^2 and bin tests need it as much as these
// functions do.  Both sources that include this file set it themselves as well; one that must not lose contraction
// elsewhere has to include this file last or restore it with `#pragma clang fp contract(on)`.
#pragma once
#pragma clang fp contract(off)
#include "fb_plan.h"
#include <algorithm>

#define FB_FOF_TILE 64                   // particles per LDS tile = lanes per workgroup of the pair search (FOF_TILE of halos.py)
#define FB_FOF_ERR_POS 1u                // error word: a position that is not finite, or too large to wrap into the box
#define FB_FOF_NONE 0xFFFFFFFFu
#define FB_FOF_WRAP_MAX 4503599627370496.0   // 2^52: positions must satisfy |x| < 2^52 L
#define FB_FOF_SCAN_PER 16
#define FB_FOF_SCAN_CH (256 * FB_FOF_SCAN_PER)

namespace {

struct FofGeom { double L[3]; double s[3]; int nc[3]; };        // box, cells per unit length, cells per axis

__device__ __forceinline__ double fof_wrap(double x, double L) {
    x = x - L * floor(x / L);
    if (x < 0.0) x += L;
    if (x >= L) x -= L;
    return x;
}
__device__ __forceinline__ double fof_min_image(double d, double L) {
    const double h = 0.5 * L;
    if (d > h) d -= L;
    else if (d < -h) d += L;
    return d;
}
__device__ __forceinline__ unsigned fof_cell(const FofGeom& g, double w0, double w1, double w2) {
    const int c0 = max(min((int)(w0 * g.s[0]), g.nc[0] - 1), 0), c1 = max(min((int)(w1 * g.s[1]), g.nc[1] - 1), 0),
              c2 = max(min((int)(w2 * g.s[2]), g.nc[2] - 1), 0);
    return ((unsigned)c0 * (unsigned)g.nc[1] + (unsigned)c1) * (unsigned)g.nc[2] + (unsigned)c2;
}

// the cell of every particle and the cells' occupancy (integer adds: any order).  A position that is not finite, that has
// |x| >= 2^52 L (floor(x / L) is no longer the integer it stands for, the wrap is meaningless), or whose wrapped value
// does not land in [0, L) all the same, sets the error word and enters no cell
__global__ __launch_bounds__(256) void k_fof_bin(const double* pos, unsigned long long n, FofGeom g, unsigned* cellid, unsigned* hist,
                                                 unsigned* err) {
    bool bad = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double x0 = pos[3 * i], x1 = pos[3 * i + 1], x2 = pos[3 * i + 2];
        const double w0 = fof_wrap(x0, g.L[0]), w1 = fof_wrap(x1, g.L[1]), w2 = fof_wrap(x2, g.L[2]);
        const bool small = fabs(x0) < FB_FOF_WRAP_MAX * g.L[0] && fabs(x1) < FB_FOF_WRAP_MAX * g.L[1] && fabs(x2) < FB_FOF_WRAP_MAX * g.L[2];
        if (!(small && w0 >= 0.0 && w0 < g.L[0] && w1 >= 0.0 && w1 < g.L[1] && w2 >= 0.0 && w2 < g.L[2])) {     // NaN fails every test
            bad = true; cellid[i] = FB_FOF_NONE; continue;
        }
        const unsigned c = fof_cell(g, w0, w1, w2);
        cellid[i] = c;
        atomicAdd(&hist[c], 1u);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, FB_FOF_ERR_POS);
}

// exclusive scan of in[0..M) into out[0..M], out[M] = the total, in three steps (after the scan of fb_halo.hip): chunk sums, a
// scan of the chunk sums in one workgroup, the chunks themselves.  The total stays below 2^32: it is the number of particles.
__device__ __forceinline__ unsigned scan_in(const unsigned* in, unsigned long long j, unsigned long long M) { return j < M ? in[j] : 0u; }
__global__ __launch_bounds__(256) void k_fof_scan_chunks(const unsigned* in, unsigned long long M, unsigned* csum) {
    const unsigned long long j0 = (unsigned long long)blockIdx.x * FB_FOF_SCAN_CH;
    unsigned s = 0;
    for (int q = 0; q < FB_FOF_SCAN_PER; ++q) s += scan_in(in, j0 + (unsigned long long)q * 256 + threadIdx.x, M);
    __shared__ unsigned tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    atomicAdd(&tot, s);
    __syncthreads();
    if (threadIdx.x == 0) csum[blockIdx.x] = tot;
}
__device__ unsigned block_exscan(unsigned v, unsigned* total) {
    __shared__ unsigned sh[256];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned a = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0u;
        __syncthreads();
        sh[threadIdx.x] += a;
        __syncthreads();
    }
    const unsigned incl = sh[threadIdx.x];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}
__global__ __launch_bounds__(256) void k_fof_scan_top(unsigned* csum, int nc) {
    unsigned carry = 0;
    for (int base = 0; base < nc; base += 256) {
        const int i = base + threadIdx.x;
        const unsigned v = i < nc ? csum[i] : 0u;
        unsigned tot;
        const unsigned ex = block_exscan(v, &tot);
        if (i < nc) csum[i] = carry + ex;
        carry += tot;
    }
}
__global__ __launch_bounds__(256) void k_fof_scan_apply(const unsigned* in, unsigned long long M, const unsigned* csum, unsigned* out) {
    const unsigned long long j0 = (unsigned long long)blockIdx.x * FB_FOF_SCAN_CH + (unsigned long long)threadIdx.x * FB_FOF_SCAN_PER;
    unsigned w[FB_FOF_SCAN_PER], s = 0;
    for (int q = 0; q < FB_FOF_SCAN_PER; ++q) { w[q] = scan_in(in, j0 + q, M); s += w[q]; }
    unsigned tot;
    unsigned run = csum[blockIdx.x] + block_exscan(s, &tot);
    for (int q = 0; q < FB_FOF_SCAN_PER; ++q) {
        if (j0 + q <= M) out[j0 + q] = run;
        run += w[q];
    }
}

// the permutation by cell and the wrapped positions in that order; every particle becomes its own root.  The order inside a
// cell is that of the atomic cursor: arbitrary, and no output depends on it.  perm and par may each be NULL: not written.
__global__ __launch_bounds__(256) void k_fof_scatter(const double* pos, unsigned long long n, FofGeom g, const unsigned* cellid,
                                                     const unsigned* start, unsigned* cursor, unsigned* perm, double* spos,
                                                     unsigned* par) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned c = cellid[i];
        const unsigned long long slot = (unsigned long long)start[c] + atomicAdd(&cursor[c], 1u);
        if (perm) perm[slot] = (unsigned)i;
        spos[3 * slot] = fof_wrap(pos[3 * i], g.L[0]);
        spos[3 * slot + 1] = fof_wrap(pos[3 * i + 1], g.L[1]);
        spos[3 * slot + 2] = fof_wrap(pos[3 * i + 2], g.L[2]);
        if (par) par[i] = (unsigned)i;
    }
}

// the tiles k >= 1 of the cells that hold more than one tile, as (cell, k) pairs in arbitrary order: at most n / TILE of them
__global__ __launch_bounds__(256) void k_fof_items(const unsigned* start, unsigned long long ncells, unsigned* items, unsigned* nitems) {
    for (unsigned long long c = (unsigned long long)blockIdx.x * 256 + threadIdx.x; c < ncells; c += (unsigned long long)gridDim.x * 256) {
        const unsigned cnt = start[c + 1] - start[c];
        for (unsigned k = 1; k * FB_FOF_TILE < cnt; ++k) {
            const unsigned slot = atomicAdd(nitems, 1u);
            items[2ull * slot] = (unsigned)c;
            items[2ull * slot + 1] = k;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
int grid_for(unsigned long long n, const fb_plan* p) {
    const unsigned long long b = (n + 255) / 256, cap = 8ull * p->num_cu * 8;
    return (int)std::max(1ull, std::min(b, cap));
}
unsigned long long scan_chunks(unsigned long long m) { return (m + FB_FOF_SCAN_CH - 1) / FB_FOF_SCAN_CH; }
size_t align16(size_t b) { return (b + 15) / 16 * 16; }
FofGeom geom_of(const fb_plan* p, const int* nc) {
    FofGeom g;
    for (int a = 0; a < 3; ++a) { g.L[a] = p->L[a]; g.nc[a] = nc ? nc[a] : 1; g.s[a] = (double)g.nc[a] / p->L[a]; }
    return g;
}

}  // namespace
