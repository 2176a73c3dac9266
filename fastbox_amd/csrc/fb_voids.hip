// Void finding (the reference's fastbox/voids.py and examples/example_void_detection.py): a steepest-descent watershed,
// per-region statistics, merging of adjacent regions of similar mean, and stacking of a field over a set of voids.  Both plan
// precisions are compiled here; see include/fastbox_hip.h for the entry points and DESIGN.md section 4 for the definitions.
//
// No contraction anywhere in this file: the stacking points, their fractional indices and the corner tests must be the doubles
// of the numpy statement (tests/voids_numpy.py), so that a point is valid on the device exactly when it is valid there.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include "fb_scan.h"
#include <algorithm>
#include <cmath>

#define FB_VOID_SMALL (1 << 16)          // bytes of void_small: [0] changed flag, [1] error word, [1] (double) bound, partials
#define FB_VOID_RED_BLOCKS 2048          // workgroups of the grid-stride reductions
#define FB_VOID_OUT 0xFFFFFFFFu          // parent word of a voxel outside the mask
#define FB_VOID_ROOT 0x80000000u         // parent word of a minimum once it holds its label
#define FB_VOID_TILE 4096                // voxels per workgroup of the minima count and rank
#define FB_VOID_MAX_JUMPS 40             // pointer-jumping rounds (path lengths halve: 2^30 voxels need 31)
// hooking rounds of the merge.  Min-label hooking has no proven logarithmic bound (a path of regions whose labels alternate can
// need more rounds); on density fields it takes 5-6 rounds (the last finds nothing to join) at 128^3, 256^3 and 512^3
// (tools/voids_bench.py).  Past the limit the call returns FB_ERR_STATE instead of looping on.
#define FB_VOID_MAX_HOOKS 64
#define FB_VOID_STACK_CHUNKS 64          // void chunks of the stacking partials

namespace {
using namespace fb;

__device__ __forceinline__ bool in_mask(int kind, double thr, const void* mp, double v, unsigned long long g, int prec) {
    if (!isfinite(v)) return false;
    switch (kind) {
        case FB_VOID_MASK_ALL: return true;
        case FB_VOID_MASK_THRESHOLD: return v <= thr;
        case FB_VOID_MASK_U8: return ((const unsigned char*)mp)[g] != 0;
        default: return prec == 4 ? ((const float*)mp)[g] != 0.0f : ((const double*)mp)[g] != 0.0;
    }
}

// ---- watershed ----------------------------------------------------------------------------------------------------------
// Steepest descent on the strict order (f, i): each voxel in the mask points to the least of itself and its in-mask face
// neighbours.  A tile of TX x TY x TZ voxels per workgroup, staged with a one-voxel halo in LDS; outside the box or the mask: NaN.
#define WS_TX 4
#define WS_TY 4
#define WS_TZ 64
#define WS_HY (WS_TY + 2)
#define WS_HZ (WS_TZ + 2)
#define WS_HALO ((WS_TX + 2) * WS_HY * WS_HZ)
template <typename T>
__global__ __launch_bounds__(256) void k_ws_descend(const T* f, int kind, double thr, const void* mp, int N, unsigned* par) {
    __shared__ T t[WS_HALO];
    const int z0 = blockIdx.x * WS_TZ, y0 = blockIdx.y * WS_TY, x0 = blockIdx.z * WS_TX;
    const unsigned long long NN = (unsigned long long)N * N;
    for (int q = threadIdx.x; q < WS_HALO; q += 256) {
        const int hz = q % WS_HZ, hy = (q / WS_HZ) % WS_HY, hx = q / (WS_HZ * WS_HY);
        const int gx = x0 + hx - 1, gy = y0 + hy - 1, gz = z0 + hz - 1;
        T v = (T)NAN;
        if (gx >= 0 && gx < N && gy >= 0 && gy < N && gz >= 0 && gz < N) {
            const unsigned long long g = (unsigned long long)gx * NN + (unsigned long long)gy * N + (unsigned long long)gz;
            const T a = f[g];
            if (in_mask(kind, thr, mp, (double)a, g, (int)sizeof(T))) v = a;
        }
        t[q] = v;
    }
    __syncthreads();
    const int off[6] = {-WS_HY * WS_HZ, WS_HY * WS_HZ, -WS_HZ, WS_HZ, -1, 1};
    const long long goff[6] = {-(long long)NN, (long long)NN, -(long long)N, (long long)N, -1, 1};
    for (int k = 0; k < WS_TX * WS_TY * WS_TZ / 256; ++k) {
        const int id = threadIdx.x + 256 * k;
        const int lz = id % WS_TZ, ly = (id / WS_TZ) % WS_TY, lx = id / (WS_TZ * WS_TY);
        const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
        if (gx >= N || gy >= N || gz >= N) continue;
        const unsigned long long g = (unsigned long long)gx * NN + (unsigned long long)gy * N + (unsigned long long)gz;
        const int c = ((lx + 1) * WS_HY + ly + 1) * WS_HZ + lz + 1;
        T bv = t[c];
        if (bv != bv) { par[g] = FB_VOID_OUT; continue; }
        long long bj = (long long)g;
        for (int d = 0; d < 6; ++d) {
            const T v = t[c + off[d]];
            const long long j = (long long)g + goff[d];
            if (v == v && (v < bv || (v == bv && j < bj))) { bv = v; bj = j; }
        }
        par[g] = (unsigned)bj;
    }
}

// one round of pointer jumping, par[i] = par[par[i]]; *changed |= 1 if some pointer moved.  A word read from another CU may be
// an older one: it is still an ancestor, and a root never changes, so "nothing moved" means every voxel points to its root.
__global__ __launch_bounds__(256) void k_ws_jump(unsigned* par, unsigned long long n, unsigned* changed) {
    bool ch = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned v = par[i];
        if (v == FB_VOID_OUT) continue;
        const unsigned w = par[v];
        if (w != v) { par[i] = w; ch = true; }
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}

// exclusive scan of v over the workgroup's 256 lanes in LDS (Hillis-Steele); `total` receives the sum
// minima (par[i] == i) per tile of FB_VOID_TILE voxels
__global__ __launch_bounds__(256) void k_ws_count(const unsigned* par, unsigned long long n, unsigned* cnt) {
    const unsigned long long b0 = (unsigned long long)blockIdx.x * FB_VOID_TILE;
    unsigned c = 0;
    for (int q = threadIdx.x; q < FB_VOID_TILE; q += 256) {
        const unsigned long long i = b0 + q;
        if (i < n && par[i] == (unsigned)i) ++c;
    }
    unsigned tot;
    (void)block_exscan(c, &tot);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// each minimum takes label 1 + its rank among all minima in raster order: the tile's offset, then 256 voxels at a time in order
__global__ __launch_bounds__(256) void k_ws_roots(unsigned* par, unsigned long long n, const unsigned* off) {
    unsigned run = off[blockIdx.x];
    const unsigned long long b0 = (unsigned long long)blockIdx.x * FB_VOID_TILE;
    for (int s0 = 0; s0 < FB_VOID_TILE; s0 += 256) {
        const unsigned long long i = b0 + s0 + threadIdx.x;
        const unsigned isr = (i < n && par[i] == (unsigned)i) ? 1u : 0u;
        unsigned tot;
        const unsigned ex = block_exscan(isr, &tot);
        if (isr) par[i] = FB_VOID_ROOT | (run + ex + 1u);
        run += tot;
    }
}

// in place: parent words -> labels (0 outside the mask).  A voxel reads only its own word and its root's, and the root's word
// holds the label with or without the root bit, whichever the order of the lanes.
__global__ __launch_bounds__(256) void k_ws_label(unsigned* par, unsigned long long n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned v = par[i];
        unsigned lab;
        if (v == FB_VOID_OUT) lab = 0u;
        else if (v & FB_VOID_ROOT) lab = v & ~FB_VOID_ROOT;
        else lab = par[v] & ~FB_VOID_ROOT;
        par[i] = lab;
    }
}

// ---- region statistics ----------------------------------------------------------------------------------------------------
// Accumulators acc (u64) [16][n1]: 0 count, 1-3 sums of the voxel indices per axis, 4 least key of f, 5 least voxel index of that
// key, 6-15 five fixed-point (hi, lo) pairs: sum f, sum w, sum w ix, sum w iy, sum w iz (w = max(-f, 0)).
// order-preserving key of a finite double (-0 is +0)
__device__ __forceinline__ unsigned long long okey(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// fixed point in two 64-bit accumulators (fb_dev.h): for a bound B (every |sum| < 2^e) values are scaled by 2^(93 - e)
__device__ __forceinline__ void fx_add(unsigned long long* hi, unsigned long long* lo, double x, double scale) {
    if (x == 0.0) return;
    unsigned long long h, l;
    fx_split(x * scale, h, l);
    atomicAdd(hi, h);
    atomicAdd(lo, l);
}
// (not fx_join: the low words are summed unsigned here and their carry, lo >> 32, moves into hi first)
__device__ __forceinline__ double fx_value(unsigned long long hi, unsigned long long lo, int F) {
    const long long h = (long long)hi + (long long)(lo >> 32);
    return ldexp((double)h * 4294967296.0 + (double)(lo & 0xFFFFFFFFull), -F);
}

// sum |f| over the finite voxels (per-workgroup partials) and the error word: 1 a voxel of label >= 1 is not finite, 2 a label
// outside 0..nl
template <typename T>
__global__ __launch_bounds__(256) void k_rs_bound(const int* lab, const T* f, unsigned long long n, long long nl, double* part,
                                                  unsigned* err) {
    double acc = 0.0;
    unsigned e = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int l = lab[i];
        if (l < 0 || (long long)l > nl) { e |= 2u; continue; }
        if (!f) continue;
        const double v = (double)f[i];
        if (isfinite(v)) acc += fabs(v);
        else if (l > 0) e |= 1u;
    }
    if (e) atomicOr(err, e);
    __shared__ double red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_rs_bound_finish(const double* part, int nb, double* out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_rs_init(unsigned long long* acc, unsigned long long n1) {
    for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < 16 * n1; j += (unsigned long long)gridDim.x * 256)
        acc[j] = (j >= 4 * n1 && j < 6 * n1) ? ~0ull : 0ull;
}

// Each wave takes 64 consecutive voxels.  Runs of equal labels over consecutive lanes are reduced first (a segmented Hillis-Steele
// scan, fixed order), and only the last lane of a run adds into the label's accumulators: one set of atomics per run, not per
// voxel.  The floating-point partials go in as fixed-point integers, so the totals do not depend on the order in which the runs
// arrive.  A non-finite voxel of label 0 adds to the count and the index sums only.
// Label 0 (outside the mask) can hold half the box, and one set of atomics per run would still send ~15 atomics per wave and per
// step to the same 15 words.  Its runs are therefore added, as the same fixed-point integers, into registers of the lane that ends
// them, and each wave adds its register totals once at the end: 15 atomics per wave for label 0 instead of 15 per 64 voxels.
template <typename T>
__global__ __launch_bounds__(256) void k_rs_accum(const int* lab, const T* f, unsigned long long n, int N, unsigned long long n1,
                                                  const double* bound, unsigned long long* acc) {
    const double B = f ? bound[0] : 0.0;
    const double s1 = ldexp(1.0, fx_exponent(B, 93)), s2 = ldexp(1.0, fx_exponent(B * (double)N, 93));
    const int lane = threadIdx.x & 63;
    const unsigned long long NN = (unsigned long long)N * N;
    unsigned long long z[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, zkey = ~0ull;    // label 0: count, ix, iy, iz, 5 x (hi, lo)
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < n; base += (unsigned long long)gridDim.x * 256) {
        const unsigned long long i = base + threadIdx.x;
        const bool ok = i < n;
        const int l = ok ? lab[i] : -1;
        unsigned long long c = ok ? 1ull : 0ull, ix = 0, iy = 0, iz = 0, key = ~0ull;
        double vf = 0.0, vw = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
        if (ok) {
            ix = i / NN; iy = (i / (unsigned)N) % (unsigned)N; iz = i % (unsigned)N;
            if (f) {
                const double v = (double)f[i];
                if (isfinite(v)) {
                    vf = v;
                    vw = fmax(-v, 0.0);
                    wx = vw * (double)ix; wy = vw * (double)iy; wz = vw * (double)iz;
                    key = okey(v);
                }
            }
        }
        const int lprev = __shfl_up(l, 1);
        const unsigned long long heads = __ballot(lane == 0 || lprev != l);
        const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const int start = 63 - __clzll((long long)(heads & upto));
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long c2 = __shfl_up(c, o), x2 = __shfl_up(ix, o), y2 = __shfl_up(iy, o), z2 = __shfl_up(iz, o);
            const unsigned long long k2 = __shfl_up(key, o);
            const double f2 = __shfl_up(vf, o), w2 = __shfl_up(vw, o), a2 = __shfl_up(wx, o), b2 = __shfl_up(wy, o),
                         d2 = __shfl_up(wz, o);
            if (lane - o >= start) {
                c += c2; ix += x2; iy += y2; iz += z2;
                key = k2 < key ? k2 : key;
                vf = f2 + vf; vw = w2 + vw; wx = a2 + wx; wy = b2 + wy; wz = d2 + wz;
            }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && l == 0) {
            z[0] += c; z[1] += ix; z[2] += iy; z[3] += iz;
            zkey = key < zkey ? key : zkey;
            const double xs[5] = {vf, vw, wx, wy, wz};
            for (int q = 0; q < 5; ++q) {
                unsigned long long h, lo;
                fx_split(xs[q] * (q < 2 ? s1 : s2), h, lo);
                z[4 + 2 * q] += h; z[5 + 2 * q] += lo;
            }
        } else if (tail && l > 0 && (unsigned long long)l < n1) {
            unsigned long long* a = acc + (unsigned long long)l;
            atomicAdd(a, c);
            atomicAdd(a + n1, ix); atomicAdd(a + 2 * n1, iy); atomicAdd(a + 3 * n1, iz);
            if (key != ~0ull) atomicMin(a + 4 * n1, key);
            fx_add(a + 6 * n1, a + 7 * n1, vf, s1);
            fx_add(a + 8 * n1, a + 9 * n1, vw, s1);
            fx_add(a + 10 * n1, a + 11 * n1, wx, s2);
            fx_add(a + 12 * n1, a + 13 * n1, wy, s2);
            fx_add(a + 14 * n1, a + 15 * n1, wz, s2);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                          // integer sums: exact in any order
        for (int k = 0; k < 14; ++k) z[k] += __shfl_xor(z[k], o);
        const unsigned long long k2 = __shfl_xor(zkey, o);
        zkey = k2 < zkey ? k2 : zkey;
    }
    if (lane == 0 && z[0]) {
        atomicAdd(acc, z[0]);
        for (int k = 1; k < 4; ++k) atomicAdd(acc + k * n1, z[k]);
        if (zkey != ~0ull) atomicMin(acc + 4 * n1, zkey);
        for (int k = 4; k < 14; ++k) atomicAdd(acc + (k + 2) * n1, z[k]);
    }
}

// the arg-min in (f, i) order: the least index among the voxels whose key is their label's least key
template <typename T>
__global__ __launch_bounds__(256) void k_rs_argmin(const int* lab, const T* f, unsigned long long n, unsigned long long n1,
                                                   unsigned long long* acc) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int l = lab[i];
        if (l < 0 || (unsigned long long)l >= n1) continue;
        const double v = (double)f[i];
        if (isfinite(v) && okey(v) == acc[4 * n1 + l]) atomicMin(&acc[5 * n1 + l], i);
    }
}

// out [FB_VOID_STAT_COLS][n1]: int64 count, arg-min (-1: none), index sums x, y, z; double sum f, sum w, sum w ix, iy, iz, mean f
__global__ __launch_bounds__(256) void k_rs_finish(const unsigned long long* acc, unsigned long long n1, int N, const double* bound,
                                                   int has_field, void* out) {
    long long* oi = (long long*)out;
    double* od = (double*)out;
    const double B = has_field ? bound[0] : 0.0;
    const int F1 = fx_exponent(B, 93), F2 = fx_exponent(B * (double)N, 93);
    for (unsigned long long l = (unsigned long long)blockIdx.x * 256 + threadIdx.x; l < n1; l += (unsigned long long)gridDim.x * 256) {
        const unsigned long long cnt = acc[l];
        oi[l] = (long long)cnt;
        oi[n1 + l] = acc[5 * n1 + l] == ~0ull ? -1ll : (long long)acc[5 * n1 + l];
        for (int a = 0; a < 3; ++a) oi[(2 + a) * n1 + l] = (long long)acc[(1 + a) * n1 + l];
        const double sf = fx_value(acc[6 * n1 + l], acc[7 * n1 + l], F1);
        od[5 * n1 + l] = sf;
        od[6 * n1 + l] = fx_value(acc[8 * n1 + l], acc[9 * n1 + l], F1);
        for (int a = 0; a < 3; ++a) od[(7 + a) * n1 + l] = fx_value(acc[(10 + 2 * a) * n1 + l], acc[(11 + 2 * a) * n1 + l], F2);
        od[10 * n1 + l] = sf / (double)cnt;
    }
}

// ---- merging --------------------------------------------------------------------------------------------------------------
// comp[l]: a label of the same component, never above l.  Hooking: for every pair of face neighbours with labels li != lj (both
// >= 1) whose means differ by less than thr, the larger of the two representatives points to the smaller (atomicMin); then
// pointer jumping to the roots.  At the fixed point every root is the least label of its component.
__global__ __launch_bounds__(256) void k_mg_init(unsigned* comp, unsigned long long n1) {
    for (unsigned long long l = (unsigned long long)blockIdx.x * 256 + threadIdx.x; l < n1; l += (unsigned long long)gridDim.x * 256)
        comp[l] = (unsigned)l;
}
__global__ __launch_bounds__(256) void k_mg_hook(const int* lab, unsigned long long n, int N, unsigned long long n1, const double* mean,
                                                 double thr, unsigned* comp, unsigned* changed) {
    bool ch = false;
    const unsigned long long NN = (unsigned long long)N * N;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int li = lab[i];
        if (li <= 0 || (unsigned long long)li >= n1) continue;
        const unsigned long long ix = i / NN, iy = (i / (unsigned)N) % (unsigned)N, iz = i % (unsigned)N;
        const bool has[3] = {ix + 1 < (unsigned long long)N, iy + 1 < (unsigned long long)N, iz + 1 < (unsigned long long)N};
        const unsigned long long step[3] = {NN, (unsigned long long)N, 1ull};
        for (int d = 0; d < 3; ++d) {
            if (!has[d]) continue;
            const int lj = lab[i + step[d]];
            if (lj <= 0 || lj == li || (unsigned long long)lj >= n1) continue;
            if (!(fabs(mean[li] - mean[lj]) < thr)) continue;
            const unsigned ci = comp[li], cj = comp[lj];
            if (ci != cj) { atomicMin(&comp[ci > cj ? ci : cj], ci < cj ? ci : cj); ch = true; }
        }
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}
__global__ __launch_bounds__(256) void k_mg_jump(unsigned* comp, unsigned long long n1, unsigned* changed) {
    bool ch = false;
    for (unsigned long long l = (unsigned long long)blockIdx.x * 256 + threadIdx.x; l < n1; l += (unsigned long long)gridDim.x * 256) {
        const unsigned c = comp[l], cc = comp[c];
        if (cc != c) { comp[l] = cc; ch = true; }
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}
__global__ __launch_bounds__(256) void k_mg_isroot(const unsigned* comp, unsigned long long n1, unsigned* flag) {
    for (unsigned long long l = (unsigned long long)blockIdx.x * 256 + threadIdx.x; l < n1; l += (unsigned long long)gridDim.x * 256)
        flag[l] = (l >= 1 && comp[l] == (unsigned)l) ? 1u : 0u;
}
// the merged label of l: 1 + the rank of its root among the roots in label order; 0 stays 0
__global__ __launch_bounds__(256) void k_mg_newlab(const unsigned* comp, const unsigned* rank, unsigned long long n1, unsigned* newlab) {
    for (unsigned long long l = (unsigned long long)blockIdx.x * 256 + threadIdx.x; l < n1; l += (unsigned long long)gridDim.x * 256)
        newlab[l] = l == 0 ? 0u : rank[comp[l]] + 1u;
}
__global__ __launch_bounds__(256) void k_mg_relabel(const int* lab, unsigned long long n, unsigned long long n1, const unsigned* newlab,
                                                    int* out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int l = lab[i];
        out[i] = (l > 0 && (unsigned long long)l < n1) ? (int)newlab[l] : 0;
    }
}

// ---- stacking -------------------------------------------------------------------------------------------------------------
// Workgroup (tile of 256 grid points, chunk of voids): each lane takes one point and the chunk's voids in order.  Point (a, b, c)
// of void v is p = c_v + R_v (grid[b], grid[a], grid[c]) (numpy's 'xy' meshgrid); u = (p - x0) / dx per axis; valid when the 8
// voxels floor(u) + {0, 1}^3 lie in the box, all carry the void's label, and the trilinear value is finite.
template <typename T>
__global__ __launch_bounds__(256) void k_stack(const int* lab, const T* f, int N, const int* vl, const double* geom, long long nv,
                                               long long chunk, const double* grid, int G, double x0, double dx, double y0,
                                               double dy, double z0, double dz, double* psum, unsigned* pcnt, int* hit) {
    const unsigned long long P = (unsigned long long)G * G * G;
    const unsigned long long pt = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = pt < P;
    const unsigned long long q = ok ? pt : 0ull;
    const int ia = (int)(q / ((unsigned long long)G * G)), ib = (int)((q / (unsigned)G) % (unsigned)G), ic = (int)(q % (unsigned)G);
    const double gx = grid[ib], gy = grid[ia], gz = grid[ic];
    const unsigned long long NN = (unsigned long long)N * N;
    const unsigned long long o[8] = {0ull, 1ull, (unsigned long long)N, (unsigned long long)N + 1, NN, NN + 1, NN + N, NN + N + 1};
    const long long v0 = (long long)blockIdx.y * chunk;
    const long long v1 = v0 + chunk < nv ? v0 + chunk : nv;
    const double top = (double)(N - 2);
    double s = 0.0;
    unsigned cnt = 0;
    for (long long v = v0; v < v1; ++v) {
        const double cx = geom[4 * v], cy = geom[4 * v + 1], cz = geom[4 * v + 2], R = geom[4 * v + 3];
        const int L = vl[v];
        bool valid = false;
        double val = 0.0;
        if (ok) {
            const double ux = ((cx + R * gx) - x0) / dx, uy = ((cy + R * gy) - y0) / dy, uz = ((cz + R * gz) - z0) / dz;
            const double fx = floor(ux), fy = floor(uy), fz = floor(uz);
            if (fx >= 0.0 && fx <= top && fy >= 0.0 && fy <= top && fz >= 0.0 && fz <= top) {      // NaN fails every test
                const unsigned long long g = (unsigned long long)fx * NN + (unsigned long long)fy * N + (unsigned long long)fz;
                valid = true;
                for (int k = 0; k < 8; ++k) valid = valid && lab[g + o[k]] == L;
                if (valid) {
                    const double tx = ux - fx, ty = uy - fy, tz = uz - fz;
                    double w[8];                                  // corner k = 4 dx + 2 dy + dz
                    for (int k = 0; k < 8; ++k) w[k] = (double)f[g + o[k]];
                    val = (1.0 - tx) * ((1.0 - ty) * ((1.0 - tz) * w[0] + tz * w[1]) + ty * ((1.0 - tz) * w[2] + tz * w[3]))
                        + tx * ((1.0 - ty) * ((1.0 - tz) * w[4] + tz * w[5]) + ty * ((1.0 - tz) * w[6] + tz * w[7]));
                    valid = isfinite(val);
                }
            }
        }
        if (valid) { s += val; ++cnt; }
        if (__any(valid) && (threadIdx.x & 63) == 0) atomicOr(&hit[v], 1);
    }
    if (ok) {
        psum[(unsigned long long)blockIdx.y * P + pt] = s;
        pcnt[(unsigned long long)blockIdx.y * P + pt] = cnt;
    }
}
// the chunks' partials in chunk order
__global__ __launch_bounds__(256) void k_stack_finish(const double* psum, const unsigned* pcnt, int nc, unsigned long long P,
                                                      double* mean, long long* count) {
    for (unsigned long long pt = (unsigned long long)blockIdx.x * 256 + threadIdx.x; pt < P; pt += (unsigned long long)gridDim.x * 256) {
        double s = 0.0;
        unsigned long long c = 0;
        for (int k = 0; k < nc; ++k) { s += psum[(unsigned long long)k * P + pt]; c += pcnt[(unsigned long long)k * P + pt]; }
        count[pt] = (long long)c;
        mean[pt] = c ? s / (double)c : (double)NAN;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
unsigned* small_flag(fb_plan* p) { return p->void_small.as<unsigned>(); }
unsigned* small_err(fb_plan* p) { return p->void_small.as<unsigned>() + 1; }
double* small_bound(fb_plan* p) { return p->void_small.as<double>() + 1; }
double* small_part(fb_plan* p) { return p->void_small.as<double>() + 8; }      // [FB_VOID_RED_BLOCKS]

template <typename T>
int watershed(fb_plan* p, const void* field, int kind, double thr, const void* mask, unsigned* par, int64_t* nreg, hipStream_t s) {
    const int N = p->N;
    const unsigned long long n = (unsigned long long)N * N * N;
    const unsigned long long nb = (n + FB_VOID_TILE - 1) / FB_VOID_TILE;
    int r = p->void_small.ensure(FB_VOID_SMALL);
    if (!r) r = p->void_work.ensure((size_t)(2 * nb + 1 + scan_chunks(nb)) * 4);
    if (r) return r;
    unsigned* cnt = p->void_work.as<unsigned>();         // [nb]
    unsigned* off = cnt + nb;                            // [nb + 1]: the scan of cnt, off[nb] = the number of minima (totals below 2^31)
    unsigned* csum = off + nb + 1;
    unsigned* flag = small_flag(p);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_ws_descend<T>), dim3((N + WS_TZ - 1) / WS_TZ, (N + WS_TY - 1) / WS_TY, (N + WS_TX - 1) / WS_TX), dim3(256),
                       0, s, (const T*)field, kind, thr, mask, N, par); }
    FB_LAUNCH_CHECK("k_ws_descend");
    for (int round = 0;; ++round) {
        if (round == FB_VOID_MAX_JUMPS) {
            fb_set_error("watershed: pointer jumping did not converge");
            return FB_ERR_STATE;
        }
        FB_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_ws_jump, dim3(grid_for(n, p)), dim3(256), 0, s, par, n, flag);
        FB_LAUNCH_CHECK("k_ws_jump");
        unsigned h = 0;
        FB_TRY(fb_read_back(&h, flag, sizeof(unsigned), s));
        if (!h) break;
    }
    hipLaunchKernelGGL(k_ws_count, dim3((unsigned)nb), dim3(256), 0, s, (const unsigned*)par, n, cnt);
    FB_LAUNCH_CHECK("k_ws_count");
    r = exscan(ScanPlain{cnt}, nb, csum, off, s);
    if (r) return r;
    hipLaunchKernelGGL(k_ws_roots, dim3((unsigned)nb), dim3(256), 0, s, par, n, (const unsigned*)off);
    FB_LAUNCH_CHECK("k_ws_roots");
    hipLaunchKernelGGL(k_ws_label, dim3(grid_for(n, p)), dim3(256), 0, s, par, n);
    FB_LAUNCH_CHECK("k_ws_label");
    unsigned tot = 0;
    FB_TRY(fb_read_back(&tot, off + nb, sizeof(unsigned), s));
    *nreg = (int64_t)tot;
    return FB_OK;
}

template <typename T>
int region_stats(fb_plan* p, const int* lab, int64_t nl, const void* field, void* out, int* bad, hipStream_t s) {
    const int N = p->N;
    const unsigned long long n = (unsigned long long)N * N * N, n1 = (unsigned long long)nl + 1;
    int r = p->void_small.ensure(FB_VOID_SMALL);
    if (!r) r = p->void_work.ensure((size_t)16 * n1 * 8);
    if (r) return r;
    unsigned long long* acc = p->void_work.as<unsigned long long>();
    const T* f = (const T*)field;
    FB_HIP(hipMemsetAsync(small_err(p), 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_rs_init, dim3(grid_for(16 * n1, p)), dim3(256), 0, s, acc, n1);
    FB_LAUNCH_CHECK("k_rs_init");
    const int nb = std::min(grid_for(n, p), FB_VOID_RED_BLOCKS);
    hipLaunchKernelGGL((k_rs_bound<T>), dim3(nb), dim3(256), 0, s, lab, f, n, (long long)nl, small_part(p), small_err(p));
    FB_LAUNCH_CHECK("k_rs_bound");
    hipLaunchKernelGGL(k_rs_bound_finish, dim3(1), dim3(256), 0, s, (const double*)small_part(p), nb, small_bound(p));
    FB_LAUNCH_CHECK("k_rs_bound_finish");
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_rs_accum<T>), dim3(grid_for(n, p)), dim3(256), 0, s, lab, f, n, N, n1, (const double*)small_bound(p), acc); }
    FB_LAUNCH_CHECK("k_rs_accum");
    if (f) {
        hipLaunchKernelGGL((k_rs_argmin<T>), dim3(grid_for(n, p)), dim3(256), 0, s, lab, f, n, n1, acc);
        FB_LAUNCH_CHECK("k_rs_argmin");
    }
    hipLaunchKernelGGL(k_rs_finish, dim3(grid_for(n1, p)), dim3(256), 0, s, (const unsigned long long*)acc, n1, N,
                       (const double*)small_bound(p), f ? 1 : 0, out);
    FB_LAUNCH_CHECK("k_rs_finish");
    unsigned e = 0;
    FB_TRY(fb_read_back(&e, small_err(p), sizeof(unsigned), s));
    *bad = (int)e;
    return FB_OK;
}

int merge_regions(fb_plan* p, const int* lab, int64_t nl, const double* mean, double thr, int* out, int64_t* nmerged, hipStream_t s) {
    const int N = p->N;
    const unsigned long long n = (unsigned long long)N * N * N, n1 = (unsigned long long)nl + 1;
    int r = p->void_small.ensure(FB_VOID_SMALL);
    if (!r) r = p->void_work.ensure((size_t)(3 * n1 + 1 + scan_chunks(n1)) * 4);
    if (r) return r;
    unsigned* comp = p->void_work.as<unsigned>();
    unsigned* flags = comp + n1;
    unsigned* rank = flags + n1;                         // [n1 + 1]: the scan of flags, rank[n1] = the number of merged regions
    unsigned* csum = rank + n1 + 1;
    unsigned* changed = small_flag(p);
    hipLaunchKernelGGL(k_mg_init, dim3(grid_for(n1, p)), dim3(256), 0, s, comp, n1);
    FB_LAUNCH_CHECK("k_mg_init");
    for (int hook = 0;; ++hook) {
        if (hook == FB_VOID_MAX_HOOKS) {
            fb_set_error("merge: hooking did not converge");
            return FB_ERR_STATE;
        }
        FB_HIP(hipMemsetAsync(changed, 0, sizeof(unsigned), s));
        { FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL(k_mg_hook, dim3(grid_for(n, p)), dim3(256), 0, s, lab, n, N, n1, mean, thr, comp, changed); }
        FB_LAUNCH_CHECK("k_mg_hook");
        unsigned h = 0;
        FB_TRY(fb_read_back(&h, changed, sizeof(unsigned), s));
        if (!h) break;
        for (int jump = 0;; ++jump) {
            if (jump == FB_VOID_MAX_JUMPS) {
                fb_set_error("merge: pointer jumping did not converge");
                return FB_ERR_STATE;
            }
            FB_HIP(hipMemsetAsync(changed, 0, sizeof(unsigned), s));
            hipLaunchKernelGGL(k_mg_jump, dim3(grid_for(n1, p)), dim3(256), 0, s, comp, n1, changed);
            FB_LAUNCH_CHECK("k_mg_jump");
            FB_TRY(fb_read_back(&h, changed, sizeof(unsigned), s));
            if (!h) break;
        }
    }
    hipLaunchKernelGGL(k_mg_isroot, dim3(grid_for(n1, p)), dim3(256), 0, s, (const unsigned*)comp, n1, flags);
    FB_LAUNCH_CHECK("k_mg_isroot");
    r = exscan(ScanPlain{flags}, n1, csum, rank, s);
    if (r) return r;
    hipLaunchKernelGGL(k_mg_newlab, dim3(grid_for(n1, p)), dim3(256), 0, s, (const unsigned*)comp, (const unsigned*)rank, n1, flags);
    FB_LAUNCH_CHECK("k_mg_newlab");
    hipLaunchKernelGGL(k_mg_relabel, dim3(grid_for(n, p)), dim3(256), 0, s, lab, n, n1, (const unsigned*)flags, out);
    FB_LAUNCH_CHECK("k_mg_relabel");
    unsigned tot = 0;
    FB_TRY(fb_read_back(&tot, rank + n1, sizeof(unsigned), s));
    *nmerged = (int64_t)tot;
    return FB_OK;
}

template <typename T>
int stack_voids(fb_plan* p, const int* lab, const void* field, const int* vl, const double* geom, int64_t nv, const double* axes,
                const double* grid, int G, double* mean, int64_t* count, int* hit, hipStream_t s) {
    const unsigned long long P = (unsigned long long)G * G * G;
    const long long nch = std::max<long long>(1, std::min<long long>(nv, FB_VOID_STACK_CHUNKS));
    const long long chunk = std::max<long long>(1, (nv + nch - 1) / nch);
    const int nc = (int)std::max<long long>(1, (nv + chunk - 1) / chunk);
    const size_t offc = ((size_t)nc * P * 8 + 255) / 256 * 256;
    FB_TRY(p->void_work.ensure(offc + (size_t)nc * P * 4));
    double* psum = p->void_work.as<double>();
    unsigned* pcnt = (unsigned*)(p->void_work.as<char>() + offc);
    FB_HIP(hipMemsetAsync(hit, 0, (size_t)std::max<long long>(nv, 1) * sizeof(int), s));
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_stack<T>), dim3((unsigned)((P + 255) / 256), (unsigned)nc), dim3(256), 0, s, lab, (const T*)field, p->N, vl,
                       geom, (long long)nv, chunk, grid, G, axes[0], axes[1], axes[2], axes[3], axes[4], axes[5], psum, pcnt, hit); }
    FB_LAUNCH_CHECK("k_stack");
    hipLaunchKernelGGL(k_stack_finish, dim3(grid_for(P, p)), dim3(256), 0, s, (const double*)psum, (const unsigned*)pcnt, nc, P, mean,
                       (long long*)count);
    FB_LAUNCH_CHECK("k_stack_finish");
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_watershed(fb_plan* p, const void* field, int mask_kind, double mask_threshold, const void* mask, int32_t* labels_out,
                 int64_t* n_regions, void* stream) {
    FB_REQUIRE(p && field && labels_out && n_regions, "null pointer");
    FB_REQUIRE(!p->comm, "void finding runs on one box on one GPU");
    FB_REQUIRE(mask_kind >= FB_VOID_MASK_ALL && mask_kind <= FB_VOID_MASK_FIELD, "mask_kind must be FB_VOID_MASK_ALL .. _FIELD");
    FB_REQUIRE(mask_kind < FB_VOID_MASK_U8 || mask, "mask: null device pointer");
    FB_REQUIRE((unsigned long long)p->N * p->N * p->N < (unsigned long long)FB_VOID_ROOT,
               "watershed: N^3 must be below 2^31 (N <= 1290): a parent word holds a voxel index in 31 bits");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, watershed<float>(p, field, mask_kind, mask_threshold, mask, (unsigned*)labels_out, n_regions, s),
                       watershed<double>(p, field, mask_kind, mask_threshold, mask, (unsigned*)labels_out, n_regions, s));
}

int fb_region_stats(fb_plan* p, const int32_t* labels, int64_t n_labels, const void* field, void* stats_out, int* bad, void* stream) {
    FB_REQUIRE(p && labels && stats_out && bad, "null pointer");
    FB_REQUIRE(!p->comm, "void finding runs on one box on one GPU");
    FB_REQUIRE(n_labels >= 0 && n_labels < (int64_t)FB_VOID_ROOT, "n_labels out of range");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, region_stats<float>(p, labels, n_labels, field, stats_out, bad, s),
                       region_stats<double>(p, labels, n_labels, field, stats_out, bad, s));
}

int fb_merge_regions(fb_plan* p, const int32_t* labels, int64_t n_labels, const double* means, double threshold, int32_t* labels_out,
                     int64_t* n_merged, void* stream) {
    FB_REQUIRE(p && labels && means && labels_out && n_merged, "null pointer");
    FB_REQUIRE(!p->comm, "void finding runs on one box on one GPU");
    FB_REQUIRE(labels != labels_out, "labels_out must not alias labels");
    FB_REQUIRE(n_labels >= 0 && n_labels < (int64_t)FB_VOID_ROOT, "n_labels out of range");
    FB_USE_DEVICE(p);
    return merge_regions(p, labels, n_labels, means, threshold, labels_out, n_merged, (hipStream_t)stream);
}

int fb_stack_voids(fb_plan* p, const int32_t* labels, const void* field, const int32_t* void_labels, const double* geom,
                   int64_t n_voids, const double* axes, const double* grid, int grid_pix, double* mean_out, int64_t* count_out,
                   int32_t* hit_out, void* stream) {
    FB_REQUIRE(p && labels && field && axes && grid && mean_out && count_out && hit_out, "null pointer");
    FB_REQUIRE(n_voids == 0 || (void_labels && geom), "null pointer");
    FB_REQUIRE(!p->comm, "void finding runs on one box on one GPU");
    FB_REQUIRE(n_voids >= 0 && grid_pix >= 1 && grid_pix <= 1024, "n_voids >= 0 and 1 <= grid_pix <= 1024");
    FB_REQUIRE(p->N >= 2, "N >= 2");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, stack_voids<float>(p, labels, field, void_labels, geom, n_voids, axes, grid, grid_pix, mean_out, count_out,
                                             hit_out, s),
                       stack_voids<double>(p, labels, field, void_labels, geom, n_voids, axes, grid, grid_pix, mean_out, count_out,
                                           hit_out, s));
}

}  // extern "C"
