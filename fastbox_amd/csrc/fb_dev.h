// Device inlines every HIP source of the library takes from here instead of copying: wave and workgroup reductions, mode and
// periodic-wrap arithmetic, the 2 x 64-bit fixed-point split, the fixed-order finish of per-workgroup partials, and the grid
// size of a grid-stride launch.  A function whose result is compared bit for bit with a numpy statement carries
// `#pragma clang fp contract(off)` inside its own body: it must not depend on the pragma state of the including source.
#pragma once
#include "fb_plan.h"

namespace fb {

// ---- modes and periodic wraps ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int mode_of(int i, int N) { return i < (N >> 1) ? i : i - N; }   // box.py:119; N/2 -> -N/2

// node index into [0, N), whatever the position held
__device__ __forceinline__ long long wrap_node(long long m, int N) {
    m %= N;
    return m < 0 ? m + N : m;
}
// position into [0, L): the numpy statement x - L * floor(x / L) (an unfused multiply and subtract), then the two guards for
// a result that rounding left outside
__device__ __forceinline__ double wrap_pos(double x, double L) {
#pragma clang fp contract(off)
    x = x - L * floor(x / L);
    if (x < 0.0) x += L;
    if (x >= L) x -= L;
    return x;
}
// nodes and weights of one axis of the mass-assignment windows, at u = x N / L cells: window 0 ngp, 1 cic, 2 tsc (fb_paint's
// header comment in include/fastbox_hip.h).  Returns the number of nodes.  Painting (fb_halo.hip) and reading the mesh back
// (fb_recon.hip) share it, so that the two are adjoint to the bit.
__device__ __forceinline__ int axis_weights(double u, int window, int N, long long (&m)[3], double (&w)[3]) {
#pragma clang fp contract(off)
    if (window == 1) {
        const double f0 = floor(u), f = u - f0;
        m[0] = wrap_node((long long)f0, N); m[1] = wrap_node((long long)f0 + 1, N);
        w[0] = 1.0 - f; w[1] = f;
        return 2;
    }
    const double c = floor(u + 0.5);
    if (window == 0) { m[0] = wrap_node((long long)c, N); w[0] = 1.0; return 1; }
    const double d = u - c, a = 0.5 - d, b = 0.5 + d;
    m[0] = wrap_node((long long)c - 1, N); m[1] = wrap_node((long long)c, N); m[2] = wrap_node((long long)c + 1, N);
    w[0] = 0.5 * (a * a); w[1] = 0.75 - d * d; w[2] = 0.5 * (b * b);
    return 3;
}

// ---- Jacobi rotation --------------------------------------------------------------------------------------------------------
// (c, s) of J = [[c, s], [-s, c]] in the (p, q) plane with (J^T A J)_pq = 0 (Golub & Van Loan, Alg. 8.4.1: the smaller root);
// returns t = s / c, with which a_pp' = a_pp - t a_pq and a_qq' = a_qq + t a_pq.  No loop: a NaN goes through as a NaN.
__device__ __forceinline__ double jacobi_rotation(double app, double aqq, double apq, double& c, double& s) {
    c = 1.0; s = 0.0;
    if (apq == 0.0) return 0.0;
    const double tau = (aqq - app) / (2.0 * apq);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));     // (tau^2 = inf: t = 0)
    c = 1.0 / sqrt(1.0 + t * t);
    s = t * c;
    return t;
}

// ---- wave reductions: over the 64 lanes, the result in every lane -----------------------------------------------------------
// float: six DPP adds (row_shr 1, 2, 4, 8, then row_bcast 15 and 31 carry the row totals forward; lanes a step does not
// reach add the `old` operand 0), total in lane 63, one v_readlane -- no LDS crossbar round trips.
__device__ __forceinline__ float wave_sum(float v) {
#define FB_DPP_ADD(ctrl, rmask, bmask) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, bmask, false))
    FB_DPP_ADD(0x111, 0xf, 0xf);     // row_shr:1
    FB_DPP_ADD(0x112, 0xf, 0xf);     // row_shr:2
    FB_DPP_ADD(0x114, 0xf, 0xe);     // row_shr:4, lanes 4..15 of each row
    FB_DPP_ADD(0x118, 0xf, 0xc);     // row_shr:8, lanes 8..15 of each row
    FB_DPP_ADD(0x142, 0xa, 0xf);     // row_bcast:15 into rows 1 and 3
    FB_DPP_ADD(0x143, 0xc, 0xf);     // row_bcast:31 into rows 2 and 3
#undef FB_DPP_ADD
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// min / max of an int over the wave (same DPP ladder as wave_sum; `old` = the identity element)
template <bool MAX>
__device__ __forceinline__ int wave_minmax(int v) {
    constexpr int ident = MAX ? (int)0x80000000 : 0x7fffffff;
#define FB_DPP_MM(ctrl, rmask, bmask) do { \
        const int o = __builtin_amdgcn_update_dpp(ident, v, ctrl, rmask, bmask, false); \
        v = MAX ? (o > v ? o : v) : (o < v ? o : v); } while (0)
    FB_DPP_MM(0x111, 0xf, 0xf);
    FB_DPP_MM(0x112, 0xf, 0xf);
    FB_DPP_MM(0x114, 0xf, 0xe);
    FB_DPP_MM(0x118, 0xf, 0xc);
    FB_DPP_MM(0x142, 0xa, 0xf);
    FB_DPP_MM(0x143, 0xc, 0xf);
#undef FB_DPP_MM
    return __builtin_amdgcn_readlane(v, 63);
}
// fp64 max / min in two forms, each the comparison its callers were written with.  wave_max is fmax (IEEE maxNum: a NaN
// loses to a number).  wave_max_cmp / wave_min_cmp take the other lane's value only where it is strictly greater / less, so
// a NaN in either place never wins and the lane's own value stands; k_reduce_real and k_min_finite document that rule.
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_cmp(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ double wave_min_cmp(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}
// 256-lane workgroup reduction; the result in every lane.  op 0: sum, 1: max
static __device__ double block_reduce(double v, int op) {
    __shared__ double red[4];
    v = op ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = op ? fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
    return r;
}

// out[q] = sum over workgroups of partial[q][workgroup]; fixed order (thread-strided chains, LDS tree).  A template only so
// that the sources that launch it (as k_bin_finish<>) emit it and the others that include this file do not
template <int = 0>
static __global__ __launch_bounds__(256) void k_bin_finish(const double* __restrict__ partial, int nblocks, int nvals,
                                                           double* __restrict__ out) {
    __shared__ double sh[256];
    const int q = blockIdx.x;
    const double* src = partial + (size_t)q * nblocks;
    double c[4] = {0, 0, 0, 0};
    int r = threadIdx.x;
    for (; r + 3 * 256 < nblocks; r += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] += src[r + u * 256];
    }
    for (int u = 0; r < nblocks; r += 256, ++u) c[u & 3] += src[r];
    sh[threadIdx.x] = (c[0] + c[1]) + (c[2] + c[3]);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[q] = sh[0];
}

// ---- fixed point in two 64-bit accumulators ---------------------------------------------------------------------------------
// A contribution x is added as the integer round(x 2^F), split into hi = floor(v 2^-32) (int64) and lo = v - hi 2^32 in
// [0, 2^32] with v = x 2^F: integer adds, so a sum does not depend on the order of its terms.  F = top - e with every |sum|
// below 2^e; top = 93 leaves hi below 2^61 (about 94 significant bits), top = 61 is the single accumulator's.  How x is scaled
// to v stays with the caller.  hi 2^32 is exact, so the split (and the join) is the same with and without contraction.
__device__ __forceinline__ int fx_exponent(double bound, int top) {
    int e = 0;
    if (bound > 0.0) (void)frexp(bound, &e);      // bound < 2^e
    return top - e;
}
__device__ __forceinline__ void fx_split(double v, unsigned long long& hi, unsigned long long& lo) {
    const double h = floor(v * 2.3283064365386963e-10);
    hi = (unsigned long long)(long long)h;
    lo = (unsigned long long)__double2ll_rn(v - h * 4294967296.0);
}
__device__ __forceinline__ double fx_join(unsigned long long hi, unsigned long long lo, int F) {
    return ldexp((double)(long long)hi * 4294967296.0 + (double)lo, -F);
}

// The kernels every fixed-point mesh shares (fb_paint, fb_grid_catalogue): the bound sum |w| (n for no weights) in per-workgroup
// partials, the one-workgroup finish of such partials in a fixed order (op 0: sum, 1: max, an empty max being 0), and the
// conversion of the accumulators to the plan's reals.  F = 61 - e with sum |w| < 2^e, so no node can overflow 62 bits; TWO
// (fp64 plans): 32 more bits, split over two accumulators.  Templates for the reason k_bin_finish is one.
template <int = 0>
static __global__ __launch_bounds__(256) void k_paint_wsum(const double* w, unsigned long long n, double* partials) {
    double acc = 0.0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256)
        acc += w ? fabs(w[i]) : 1.0;
    acc = block_reduce(acc, 0);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
template <int = 0>
static __global__ __launch_bounds__(256) void k_halo_finish(const double* partials, int nb, int op, double* out) {
    double acc = op ? -INFINITY : 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc = op ? fmax(acc, partials[i]) : acc + partials[i];
    acc = block_reduce(acc, op);
    if (threadIdx.x == 0) out[0] = op && !(acc > -INFINITY) ? 0.0 : acc;
}
template <typename T, bool TWO>
static __global__ __launch_bounds__(256) void k_paint_finish(const unsigned long long* acc_hi, const unsigned long long* acc_lo,
                                                             unsigned long long n, const double* wsum, T* out) {
    const int F = fx_exponent(wsum[0], 61) + (TWO ? 32 : 0);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        out[i] = (T)(TWO ? fx_join(acc_hi[i], acc_lo[i], F) : ldexp((double)(long long)acc_hi[i], -F));
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// workgroups of 256 lanes for a grid-stride loop over n elements: one per 256 elements, at most 64 per compute unit
inline int grid_for(unsigned long long n, const fb_plan* p) {
    const unsigned long long b = (n + 255) / 256, cap = 8ull * p->num_cu * 8;
    const unsigned long long g = b < cap ? b : cap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace fb
