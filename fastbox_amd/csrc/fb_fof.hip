// Friends-of-friends halo finding on a particle set (nbodykit's FOF): cell binning, the pair search with a
// union-find over the particles, the flattening of the forest, group sizes and the catalogue of the groups kept.  Particle data
// are fp64 whatever the plan's precision; the plan gives the box and the device.  See include/fastbox_hip.h for the entry points.
//
// No contraction anywhere in this file: the wrapped positions, the minimum-image differences and d^2 = (dx dx + dy dy) + dz dz
// must be the doubles of the numpy statement (tests/fof_numpy.py), so that a pair is linked on the device exactly when it is there.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_cells.h"                    // FofGeom, wrapping, the cell binning kernels and k_fof_items: shared with fb_pairs.hip
#include <algorithm>
#include <cmath>
#include <cstring>

#define FB_FOF_SMALL 256                 // bytes at the head of every work buffer: the words below
#define FB_FOF_MAX_JUMPS 40              // pointer-jumping rounds of the flattening (path lengths halve: 2^31 particles need 32)
#define FB_FOF_ERR_LOOP 2u               // error word (FB_FOF_ERR_POS = 1 and FB_FOF_ERR_VEL = 4 are in fb_cells.h): a loop hit its cap

namespace {

// words of the small block: u32 [0] error, [1] changed, [2] items / kept; u64 [2] groups; double [3] max |v|
struct FofSmall { unsigned err, changed, count, pad; unsigned long long groups; unsigned long long vmax_bits; };

// ---- 2. pair search and union ---------------------------------------------------------------------------------------------
// Union-find over par[]: par[i] <= i always (the larger root is hooked under the smaller), so the forest has no cycle and the
// root of a finished group is its least member.  Every access to par in this kernel is a relaxed agent-scope atomic: the
// compiler cannot keep a word in a register, and no load is served by a CU's own L1.  A word that is older than the newest
// one is still an ancestor (the argument above k_ws_jump of fb_voids.hip): only a successful compare-and-swap on a true root
// changes the forest, path halving writes ancestors into non-roots only, and a node that stops being a root never becomes
// one again -- so a stale read costs steps, never a wrong link.
__device__ __forceinline__ unsigned par_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void par_store(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see, with path halving; FB_FOF_NONE (and the error word) past the cap.  Every word
// ever stored in par[i] is <= i, so each step that does not return moves x to a strictly smaller index (g <= p < x): a find
// takes at most n steps, and cap = n + 1 is reached only if the forest is corrupt.
__device__ unsigned fof_find(unsigned* par, unsigned x, unsigned cap, unsigned* err) {
    for (unsigned it = 0; it < cap; ++it) {
        const unsigned p = par_load(par + x);
        if (p == x) return x;
        const unsigned g = par_load(par + p);
        if (g != p) par_store(par + x, g);
        x = g;
    }
    atomicOr(err, FB_FOF_ERR_LOOP);
    return FB_FOF_NONE;
}
// join the groups of a and b: hook the larger root under the smaller by compare-and-swap on the larger root's own word.  A
// failure means that root was hooked elsewhere in between: go on from the parent the swap returned (a true one, not a cached
// one).  That parent and `small` are both below `big`, so the larger root of the next attempt is strictly smaller: at most n
// attempts, the same cap.
__device__ void fof_union(unsigned* par, unsigned a, unsigned b, unsigned cap, unsigned* err) {
    for (unsigned it = 0; it < cap; ++it) {
        a = fof_find(par, a, cap, err);
        b = fof_find(par, b, cap, err);
        if (a == FB_FOF_NONE || b == FB_FOF_NONE || a == b) return;
        const unsigned big = a > b ? a : b, small = a > b ? b : a;
        const unsigned old = atomicCAS(par + big, big, small);
        if (old == big) return;
        a = small; b = old;
    }
    atomicOr(err, FB_FOF_ERR_LOOP);
}

// One workgroup of one wave per (cell, home tile): the home tile and, tile by tile, the particles of the cell itself and of its
// neighbour cells go through LDS; the TILE x TILE pairs are spread over the lanes.  Every pair is decided by its own
// minimum-image d^2, not by a shift per cell, so a neighbour cell met twice (fewer than 3 cells along an axis: +1 and -1 are the
// same cell) only repeats unions that are already done.  half != 0 (3 or more cells on every axis): the cell itself and the 13
// neighbours of the upper half shell, each adjacent pair of cells once; else all 27 offsets.  Inside one cell a pair is taken
// once, by its slots.  items NULL: work item w is tile 0 of cell w; else the (cell, tile) pair items[2 w], items[2 w + 1].
__global__ __launch_bounds__(FB_FOF_TILE) void k_fof_link(FofGeom g, const unsigned* start, const unsigned* perm, const double* spos,
                                                          unsigned* par, double ell2, const unsigned* items, unsigned long long total,
                                                          int half, unsigned cap, unsigned* err) {
    __shared__ double hx[FB_FOF_TILE], hy[FB_FOF_TILE], hz[FB_FOF_TILE], nx[FB_FOF_TILE], ny[FB_FOF_TILE], nz[FB_FOF_TILE];
    __shared__ unsigned hid[FB_FOF_TILE], nid[FB_FOF_TILE];
    const int t = threadIdx.x;
    for (unsigned long long w = blockIdx.x; w < total; w += gridDim.x) {
        const unsigned c = items ? items[2 * w] : (unsigned)w, k = items ? items[2 * w + 1] : 0u;
        const unsigned b0 = start[c], b1 = start[c + 1];
        if (b1 - b0 <= k * FB_FOF_TILE) continue;                     // an empty cell: the whole workgroup skips it
        const unsigned h0 = b0 + k * FB_FOF_TILE;
        const int nh = (int)min(b1 - h0, (unsigned)FB_FOF_TILE);
        __syncthreads();
        if (t < nh) {
            hx[t] = spos[3ull * (h0 + t)]; hy[t] = spos[3ull * (h0 + t) + 1]; hz[t] = spos[3ull * (h0 + t) + 2];
            hid[t] = perm[h0 + t];
        }
        const int c2 = (int)(c % (unsigned)g.nc[2]), c1 = (int)((c / (unsigned)g.nc[2]) % (unsigned)g.nc[1]),
                  c0 = (int)(c / ((unsigned)g.nc[2] * (unsigned)g.nc[1]));
        for (int o = half ? 13 : 0; o < 27; ++o) {
            const int m0 = (c0 + o / 9 - 1 + g.nc[0]) % g.nc[0], m1 = (c1 + (o / 3) % 3 - 1 + g.nc[1]) % g.nc[1],
                      m2 = (c2 + o % 3 - 1 + g.nc[2]) % g.nc[2];
            const unsigned m = ((unsigned)m0 * (unsigned)g.nc[1] + (unsigned)m1) * (unsigned)g.nc[2] + (unsigned)m2;
            const bool same = m == c;
            const unsigned e0 = start[m], e1 = start[m + 1];
            for (unsigned q0 = e0; q0 < e1; q0 += FB_FOF_TILE) {
                const int nn = (int)min(e1 - q0, (unsigned)FB_FOF_TILE);
                __syncthreads();
                if (t < nn) {
                    nx[t] = spos[3ull * (q0 + t)]; ny[t] = spos[3ull * (q0 + t) + 1]; nz[t] = spos[3ull * (q0 + t) + 2];
                    nid[t] = perm[q0 + t];
                }
                __syncthreads();
                const int np = nh * nn;
                for (int q = t; q < np; q += FB_FOF_TILE) {
                    const int i = q / nn, j = q - i * nn;
                    if (same && h0 + (unsigned)i >= q0 + (unsigned)j) continue;
                    const double dx = fof_min_image(hx[i] - nx[j], g.L[0]), dy = fof_min_image(hy[i] - ny[j], g.L[1]),
                                 dz = fof_min_image(hz[i] - nz[j], g.L[2]);
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < ell2) fof_union(par, hid[i], nid[j], cap, err);
                }
            }
        }
    }
}

// ---- 3. flatten -----------------------------------------------------------------------------------------------------------
// one round of pointer jumping between launches, par[i] = par[par[i]]; *changed |= 1 if some pointer moved (k_ws_jump)
__global__ __launch_bounds__(256) void k_fof_jump(unsigned* par, unsigned long long n, unsigned* changed) {
    bool ch = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned v = par[i];
        const unsigned w = par[v];
        if (w != v) { par[i] = w; ch = true; }
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}

// ---- 4. sizes and catalogue ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fof_count(const unsigned* root, unsigned long long n, unsigned* count) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256)
        atomicAdd(&count[root[i]], 1u);
}
// the number of roots, and the (root, count) pairs of the groups of nmin members or more, in arbitrary order
__global__ __launch_bounds__(256) void k_fof_tally(const unsigned* root, const unsigned* count, unsigned long long n, unsigned nmin,
                                                   unsigned* kept, unsigned* nkept, unsigned long long* groups) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        if (root[i] != (unsigned)i) continue;
        atomicAdd(groups, 1ull);
        if (count[i] >= nmin) {
            const unsigned slot = atomicAdd(nkept, 1u);
            kept[2ull * slot] = (unsigned)i;
            kept[2ull * slot + 1] = count[i];
        }
    }
}

__global__ __launch_bounds__(256) void k_fof_rank(const unsigned* sroot, unsigned nk, int* labels) {
    const unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r < nk) labels[sroot[r]] = (int)r;
}
// labels holds -1 everywhere but on the roots of the groups kept (k_fof_rank); the members copy their root's word
__global__ __launch_bounds__(256) void k_fof_label(const unsigned* root, unsigned long long n, int* labels) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned r = root[i];
        if (r != (unsigned)i) labels[i] = labels[r];
    }
}
// Fixed point in two 64-bit accumulators (fb_dev.h): the sums do not depend on the order of the particles.  F = 93 - e with
// (number of particles) (bound of |x|) < 2^e: hi stays below 2^61.
__device__ __forceinline__ void fof_add(unsigned long long* acc, double x, int F) {
    unsigned long long hi, lo;
    fx_split(ldexp(x, F), hi, lo);
    atomicAdd(acc, hi);
    atomicAdd(acc + 1, lo);
}
// acc[g][6][2]: per group kept, the sums of the minimum-image offsets from the root's wrapped position and of the velocities
__global__ __launch_bounds__(256) void k_fof_accum(const double* pos, const double* vel, const unsigned* root, const int* labels,
                                                   unsigned long long n, FofGeom g, int Fp, const unsigned long long* vmax_bits,
                                                   unsigned long long* acc) {
    const int Fv = vel ? fx_exponent((double)n * __longlong_as_double((long long)vmax_bits[0]), 93) : 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int lab = labels[i];
        if (lab < 0) continue;
        const unsigned long long r = root[i];
        unsigned long long* a = acc + 12ull * (unsigned)lab;
        for (int c = 0; c < 3; ++c) {
            const double d = fof_min_image(wrap_pos(pos[3 * i + c], g.L[c]) - wrap_pos(pos[3 * r + c], g.L[c]), g.L[c]);
            fof_add(a + 2 * c, d, Fp);
            if (vel) fof_add(a + 6 + 2 * c, vel[3 * i + c], Fv);
        }
    }
}
__global__ __launch_bounds__(256) void k_fof_finish(const double* pos, const unsigned* sroot, const unsigned* scount, unsigned nk,
                                                    FofGeom g, int Fp, const unsigned long long* vmax_bits, unsigned long long n,
                                                    const unsigned long long* acc, double* com, double* vmean) {
    const unsigned r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    const int Fv = vmean ? fx_exponent((double)n * __longlong_as_double((long long)vmax_bits[0]), 93) : 0;
    const double m = (double)scount[r];
    const unsigned long long i = sroot[r];
    for (int c = 0; c < 3; ++c) {
        const double a = wrap_pos(pos[3 * i + c], g.L[c]);
        com[3ull * r + c] = wrap_pos(a + fx_join(acc[12ull * r + 2 * c], acc[12ull * r + 2 * c + 1], Fp) / m, g.L[c]);
        if (vmean) vmean[3ull * r + c] = fx_join(acc[12ull * r + 6 + 2 * c], acc[12ull * r + 6 + 2 * c + 1], Fv) / m;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the work buffer of fb_fof_link: small | spos f64[3 n] | start u32[ncells + 1] | cursor u32[ncells] | csum u32[chunks] |
// cellid u32[n] | perm u32[n] | items u32[2 (n / TILE + 1)]
struct FofWork { size_t spos, start, cursor, csum, cellid, perm, items, total; };
FofWork work_layout(unsigned long long n, unsigned long long ncells) {
    FofWork w;
    size_t o = FB_FOF_SMALL;
    w.spos = o; o += align16((size_t)n * 24);
    w.start = o; o += align16((size_t)(ncells + 1) * 4);
    w.cursor = o; o += align16((size_t)ncells * 4);
    w.csum = o; o += align16((size_t)scan_chunks(ncells) * 4);
    w.cellid = o; o += align16((size_t)n * 4);
    w.perm = o; o += align16((size_t)n * 4);
    w.items = o; o += align16((size_t)(n / FB_FOF_TILE + 1) * 8);
    w.total = o;
    return w;
}
int loop_error() {
    fb_set_error("friends-of-friends: a find or union loop hit its iteration cap");
    return FB_ERR_STATE;
}

}  // namespace

extern "C" {

int64_t fb_fof_work_bytes(int64_t n, int64_t ncells) {
    if (n < 0 || ncells < 1) return -1;
    return (int64_t)work_layout((unsigned long long)n, (unsigned long long)ncells).total;
}

int fb_fof_link(fb_plan* p, const double* pos, int64_t n, double link, const int* ncell, void* work, int64_t work_bytes,
                uint32_t* root_out, int* bad, double* stage_ms, void* stream) {
    FB_REQUIRE(p && ncell && bad, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll, "friends-of-friends: 0 <= n <= 2^31 - 2");
    const double lmin = std::min(p->L[0], std::min(p->L[1], p->L[2]));
    FB_REQUIRE(link > 0.0 && link < 0.5 * lmin, "friends-of-friends: 0 < linking length < min(L) / 2");
    unsigned long long ncells = 1;
    for (int a = 0; a < 3; ++a) {
        FB_REQUIRE(ncell[a] >= 1 && p->L[a] / (double)ncell[a] >= link, "friends-of-friends: cells of side >= the linking length");
        ncells *= (unsigned long long)ncell[a];
        FB_REQUIRE(ncells <= (1ull << 31), "friends-of-friends: at most 2^31 cells");
    }
    *bad = 0;
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = stage_ms[3] = 0.0;
    if (n == 0) return FB_OK;
    FB_REQUIRE(pos && work && root_out, "null pointer");
    const FofWork w = work_layout((unsigned long long)n, ncells);
    FB_REQUIRE(work_bytes >= (int64_t)w.total, "friends-of-friends: work buffer smaller than fb_fof_work_bytes");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    char* wb = (char*)work;
    FofSmall* sm = (FofSmall*)wb;
    double* spos = (double*)(wb + w.spos);
    unsigned *start = (unsigned*)(wb + w.start), *cursor = (unsigned*)(wb + w.cursor), *csum = (unsigned*)(wb + w.csum),
             *cellid = (unsigned*)(wb + w.cellid), *perm = (unsigned*)(wb + w.perm), *items = (unsigned*)(wb + w.items);
    const FofGeom g = geom_of(p, ncell);
    const unsigned long long un = (unsigned long long)n;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (stage_ms) for (int q = 0; q < 5; ++q) FB_HIP(hipEventCreate(&ev[q]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int q = 0; q < 5; ++q) if (e[q]) (void)hipEventDestroy(e[q]); } } evg{ev};
    if (stage_ms) FB_HIP(hipEventRecord(ev[0], s));
    // 1. bin
    FB_HIP(hipMemsetAsync(sm, 0, FB_FOF_SMALL, s));
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_bin, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, cellid, cursor, &sm->err);
    FB_LAUNCH_CHECK("k_fof_bin");
    FofSmall h;
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    if (h.err & FB_FOF_ERR_POS) { *bad = 1; return FB_OK; }          // before any linking
    FB_TRY(exscan(ScanPlain{cursor}, ncells, csum, start, s));       // start[ncells] = n
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_scatter, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, (const unsigned*)cellid, (const unsigned*)start,
                       cursor, perm, spos, (unsigned*)root_out);
    FB_LAUNCH_CHECK("k_fof_scatter");
    hipLaunchKernelGGL(k_fof_items, dim3(grid_for(ncells, p)), dim3(256), 0, s, (const unsigned*)start, ncells, items, &sm->count);
    FB_LAUNCH_CHECK("k_fof_items");
    if (stage_ms) FB_HIP(hipEventRecord(ev[1], s));
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    const unsigned long long nitems = h.count;
    // 2. link: tile 0 of every cell, then the further tiles of the crowded cells
    const int half = ncell[0] >= 3 && ncell[1] >= 3 && ncell[2] >= 3;
    const unsigned long long wgmax = 256ull * (unsigned long long)p->num_cu;
    hipLaunchKernelGGL(k_fof_link, dim3((unsigned)std::min(ncells, wgmax)), dim3(FB_FOF_TILE), 0, s, g, (const unsigned*)start,
                       (const unsigned*)perm, (const double*)spos, (unsigned*)root_out, link * link, (const unsigned*)nullptr, ncells,
                       half, (unsigned)n + 1u, &sm->err);
    FB_LAUNCH_CHECK("k_fof_link");
    if (stage_ms) FB_HIP(hipEventRecord(ev[2], s));
    if (nitems) {
        hipLaunchKernelGGL(k_fof_link, dim3((unsigned)std::min(nitems, wgmax)), dim3(FB_FOF_TILE), 0, s, g, (const unsigned*)start,
                           (const unsigned*)perm, (const double*)spos, (unsigned*)root_out, link * link, (const unsigned*)items,
                           nitems, half, (unsigned)n + 1u, &sm->err);
        FB_LAUNCH_CHECK("k_fof_link");
    }
    if (stage_ms) FB_HIP(hipEventRecord(ev[3], s));
    // 3. flatten
    for (int round = 0;; ++round) {
        if (round == FB_FOF_MAX_JUMPS) {
            fb_set_error("friends-of-friends: pointer jumping did not converge");
            return FB_ERR_STATE;
        }
        FB_HIP(hipMemsetAsync(&sm->changed, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_fof_jump, dim3(grid_for(un, p)), dim3(256), 0, s, (unsigned*)root_out, un, &sm->changed);
        FB_LAUNCH_CHECK("k_fof_jump");
        FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
        if (h.err & FB_FOF_ERR_LOOP) return loop_error();
        if (!h.changed) break;
    }
    if (stage_ms) {
        FB_HIP(hipEventRecord(ev[4], s));
        FB_HIP(hipEventSynchronize(ev[4]));
        for (int q = 0; q < 4; ++q) {
            float ms = 0.f;
            FB_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            stage_ms[q] = (double)ms;
        }
    }
    return FB_OK;
}

int fb_fof_sizes(fb_plan* p, const uint32_t* root, int64_t n, int64_t nmin, void* work, uint32_t* count_out, uint32_t* kept_out,
                 int64_t* out_host, void* stream) {
    FB_REQUIRE(p && out_host, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll && nmin >= 1, "friends-of-friends: 0 <= n <= 2^31 - 2, nmin >= 1");
    out_host[0] = out_host[1] = 0;
    if (n == 0) return FB_OK;
    FB_REQUIRE(root && work && count_out && (kept_out || nmin > n), "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    FofSmall* sm = (FofSmall*)work;
    const unsigned long long un = (unsigned long long)n;
    FB_HIP(hipMemsetAsync(sm, 0, FB_FOF_SMALL, s));
    FB_HIP(hipMemsetAsync(count_out, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(k_fof_count, dim3(grid_for(un, p)), dim3(256), 0, s, (const unsigned*)root, un, (unsigned*)count_out);
    FB_LAUNCH_CHECK("k_fof_count");
    hipLaunchKernelGGL(k_fof_tally, dim3(grid_for(un, p)), dim3(256), 0, s, (const unsigned*)root, (const unsigned*)count_out, un,
                       (unsigned)std::min<int64_t>(nmin, 0xFFFFFFFFll), (unsigned*)kept_out, &sm->count, &sm->groups);
    FB_LAUNCH_CHECK("k_fof_tally");
    FofSmall h;
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    out_host[0] = (int64_t)h.groups;
    out_host[1] = (int64_t)h.count;
    return FB_OK;
}

int fb_fof_catalogue(fb_plan* p, const double* pos, const double* vel, const uint32_t* root, int64_t n, const uint32_t* sorted_roots,
                     const uint32_t* sorted_counts, int64_t n_kept, void* work, int32_t* labels_out, double* pos_out, double* vel_out,
                     int* bad, void* stream) {
    FB_REQUIRE(p && bad, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll && n_kept >= 0 && n_kept <= n, "friends-of-friends: 0 <= n_kept <= n <= 2^31 - 2");
    *bad = 0;
    if (n == 0) return FB_OK;
    FB_REQUIRE(pos && root && labels_out, "null pointer");
    FB_REQUIRE(n_kept == 0 || (sorted_roots && sorted_counts && work && pos_out && (vel_out || !vel)), "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long un = (unsigned long long)n;
    FB_HIP(hipMemsetAsync(labels_out, 0xFF, (size_t)n * 4, s));
    if (n_kept == 0) return FB_OK;
    const unsigned nk = (unsigned)n_kept;
    FofSmall* sm = (FofSmall*)work;
    unsigned long long* acc = (unsigned long long*)((char*)work + FB_FOF_SMALL);
    const FofGeom g = geom_of(p, nullptr);
    FB_HIP(hipMemsetAsync(work, 0, FB_FOF_SMALL + (size_t)nk * 96, s));
    hipLaunchKernelGGL(k_fof_rank, dim3((nk + 255) / 256), dim3(256), 0, s, (const unsigned*)sorted_roots, nk, (int*)labels_out);
    FB_LAUNCH_CHECK("k_fof_rank");
    hipLaunchKernelGGL(k_fof_label, dim3(grid_for(un, p)), dim3(256), 0, s, (const unsigned*)root, un, (int*)labels_out);
    FB_LAUNCH_CHECK("k_fof_label");
    if (vel) {
        hipLaunchKernelGGL(k_fof_vmax, dim3(grid_for(3 * un, p)), dim3(256), 0, s, vel, 3 * un, &sm->vmax_bits, &sm->err);
        FB_LAUNCH_CHECK("k_fof_vmax");
        FofSmall h;
        FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
        double vmax;
        memcpy(&vmax, &h.vmax_bits, sizeof(vmax));
        if ((h.err & FB_FOF_ERR_VEL) || !std::isfinite((double)n * vmax)) { *bad = 4; return FB_OK; }     // the sums' bound
    }
    // sum |offset| < n max(L) / 2 < 2^e
    int e = 0;
    (void)frexp((double)n * 0.5 * std::max(p->L[0], std::max(p->L[1], p->L[2])), &e);
    const int Fp = 93 - e;
    hipLaunchKernelGGL(k_fof_accum, dim3(grid_for(un, p)), dim3(256), 0, s, pos, vel, (const unsigned*)root, (const int*)labels_out, un, g,
                       Fp, (const unsigned long long*)&sm->vmax_bits, acc);
    FB_LAUNCH_CHECK("k_fof_accum");
    hipLaunchKernelGGL(k_fof_finish, dim3((nk + 255) / 256), dim3(256), 0, s, pos, (const unsigned*)sorted_roots,
                       (const unsigned*)sorted_counts, nk, g, Fp, (const unsigned long long*)&sm->vmax_bits, un,
                       (const unsigned long long*)acc, pos_out, vel ? vel_out : nullptr);
    FB_LAUNCH_CHECK("k_fof_finish");
    return FB_OK;
}

}  // extern "C"
