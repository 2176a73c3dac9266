// Cell binning of a periodic particle set, shared by the friends-of-friends search (fb_fof.hip), the pair counts
// (fb_pairs.hip) and the halo profiles (fb_profiles.hip): minimum-image differences, the cell of a particle, the occupancy
// histogram, the permuted copy of the wrapped positions, the list of the further tiles of crowded cells and the largest |v|
// of a velocity array.  The wrap itself is wrap_pos of fb_dev.h, the scan of the histogram is exscan of fb_scan.h (both
// included here).
//
// No contraction: the wrapped positions and the minimum-image differences must be the doubles of the numpy statements
// (tests/fof_numpy.py, tests/pairs_numpy.py).  The pragma below is at file scope on purpose: it switches contraction off for
// the rest of any source that includes this file, because the callers' own d^2 and bin tests need it as much as these
// functions do.  Both sources that include this file set it themselves as well; one that must not lose contraction
// elsewhere has to include this file last or restore it with `#pragma clang fp contract(on)`.
#pragma once
#pragma clang fp contract(off)
#include "fb_plan.h"
#include "fb_dev.h"
#include "fb_scan.h"
#include <algorithm>

#define FB_FOF_TILE 64                   // particles per LDS tile = lanes per workgroup of the pair search (FOF_TILE of halos.py)
#define FB_FOF_ERR_POS 1u                // error word: a position that is not finite, or too large to wrap into the box
#define FB_FOF_ERR_VEL 4u                // error word: a velocity that is not finite
#define FB_FOF_NONE 0xFFFFFFFFu
#define FB_FOF_WRAP_MAX 4503599627370496.0   // 2^52: positions must satisfy |x| < 2^52 L

namespace {
using namespace fb;

struct FofGeom { double L[3]; double s[3]; int nc[3]; };        // box, cells per unit length, cells per axis

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
        const double w0 = wrap_pos(x0, g.L[0]), w1 = wrap_pos(x1, g.L[1]), w2 = wrap_pos(x2, g.L[2]);
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

// the permutation by cell and the wrapped positions in that order; every particle becomes its own root.  The order inside a
// cell is that of the atomic cursor: arbitrary, and no output depends on it.  perm and par may each be NULL: not written.
__global__ __launch_bounds__(256) void k_fof_scatter(const double* pos, unsigned long long n, FofGeom g, const unsigned* cellid,
                                                     const unsigned* start, unsigned* cursor, unsigned* perm, double* spos,
                                                     unsigned* par) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned c = cellid[i];
        const unsigned long long slot = (unsigned long long)start[c] + atomicAdd(&cursor[c], 1u);
        if (perm) perm[slot] = (unsigned)i;
        spos[3 * slot] = wrap_pos(pos[3 * i], g.L[0]);
        spos[3 * slot + 1] = wrap_pos(pos[3 * i + 1], g.L[1]);
        spos[3 * slot + 2] = wrap_pos(pos[3 * i + 2], g.L[2]);
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

// max |v| over all components (the bit pattern of a non-negative double orders as an integer)
__global__ __launch_bounds__(256) void k_fof_vmax(const double* vel, unsigned long long n3, unsigned long long* vmax_bits, unsigned* err) {
    double m = 0.0;
    bool bad = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256) {
        const double a = fabs(vel[i]);
        if (!(a < INFINITY)) bad = true; else m = fmax(m, a);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(vmax_bits, (unsigned long long)__double_as_longlong(m));
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(err, FB_FOF_ERR_VEL);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
size_t align16(size_t b) { return (b + 15) / 16 * 16; }
FofGeom geom_of(const fb_plan* p, const int* nc) {
    FofGeom g;
    for (int a = 0; a < 3; ++a) { g.L[a] = p->L[a]; g.nc[a] = nc ? nc[a] : 1; g.s[a] = (double)g.nc[a] / p->L[a]; }
    return g;
}

}  // namespace
