// Halo tracers (the reference's fastbox/halos.py and the painting step of examples/example_halos.py): the expected count per
// voxel and its Poisson draw, the halo catalogue in the reference's order, and mass assignment onto the mesh.
// Both plan precisions are compiled here; see include/fastbox_hip.h for the definitions and DESIGN.md for the algorithms.
//
// No contraction anywhere in this file: the fp64 expected count must be the reference's numpy expression bit for bit, and
// the Poisson inversion is reproduced by the host model fastbox_amd/rng.py.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include "fb_scan.h"
#include "fb_rng.h"
#include <algorithm>
#include <cmath>

#define FB_HALO_SMALL (1 << 16)          // bytes of halo_small: 2048 workgroups x 4 words
#define FB_HALO_RED_BLOCKS 2048          // workgroups of the grid-stride reductions
#define FB_HALO_TILE_MIN 4096            // voxels per workgroup of the catalogue
#define FB_HALO_TABLE_MAX (1ull << 25)   // (count, workgroup) entries of the catalogue's tables
#define FB_HALO_LAM_MAX 16777216.0       // 2^24: every count below it is exact in fp32

namespace {
using namespace fb;

// nbar / bias: a scalar, a profile along z (fp64 [N]), a field of the plan's precision or an fp64 field ([N^3])
struct HPrm { const void* p; double v; int kind; };
template <typename T>
__device__ __forceinline__ double hprm_at(const HPrm& q, unsigned long long i, int iz) {
    switch (q.kind) {
        case FB_HALO_SCALAR: return q.v;
        case FB_HALO_ZPROFILE: return ((const double*)q.p)[iz];
        case FB_HALO_FIELD: return (double)((const T*)q.p)[i];
        default: return ((const double*)q.p)[i];
    }
}

// log-normal statistics: per-workgroup max of bias*delta (op 1) or sum of exp(bias*delta - shift[0]) (op 0)
template <typename T>
__global__ __launch_bounds__(256) void k_halo_ln_reduce(const T* dx, HPrm bias, unsigned long long n, int N, int op,
                                                        const double* shift, double* partials) {
    const double s = op ? 0.0 : shift[0];
    double acc = op ? -INFINITY : 0.0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double dh = __dmul_rn(hprm_at<T>(bias, i, (int)(i % (unsigned)N)), (double)dx[i]);
        if (op) acc = fmax(acc, dh); else acc += exp(dh - s);
    }
    acc = block_reduce(acc, op);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
// (k_halo_finish<> of fb_dev.h: one workgroup, out[0] = reduction of partials[0..nb) in a fixed order)

// Poisson variate by inversion of the CDF with one uniform u in (0, 1), in fp64.  The search starts at the mode
// m = floor(lam) with pmf exp(m ln lam - lam - lgamma(m + 1)); the mass below the mode is summed downwards until a term falls
// below 1e-20; then the CDF is walked down or up from the mode: O(sqrt lam) steps.  Reproduced step by step by
// fastbox_amd/rng.py poisson_inverse.
__device__ double poisson_inverse(double lam, double u) {
    if (!(lam > 0.0)) return 0.0;
    const double m = floor(lam);
    const double pm = exp((m * log(lam) - lam) - lgamma(m + 1.0));
    double L = 0.0, p = pm, j = m;
    while (j > 0.0) {
        p = p * j / lam; j -= 1.0; L += p;
        if (p < 1e-20) break;
    }
    if (u < L) {                                   // below the mode: c = F(k - 1) on entry
        double k = m, c = L;
        p = pm;
        while (k > 0.0) {
            p = p * k / lam; k -= 1.0;
            if (u >= c - p) return k;
            c -= p;
        }
        return 0.0;
    }
    double k = m, c = L + pm;
    p = pm;
    while (u >= c) {
        p = p * lam / (k + 1.0); k += 1.0; c += p;
        if (p == 0.0) break;                       // past the representable tail (u within rounding of 1)
    }
    return k;
}
// the uniform of voxel i (stream 5): 53 bits of words 0 and 1, (w + 1/2) 2^-53
__device__ __forceinline__ double poisson_uniform(unsigned long long i, const fb::RngKey& key) {
    uint32_t o[4];
    fb::philox4x32(i, 5u, key, o);
    const unsigned long long w = ((unsigned long long)o[0] << 21) | (unsigned long long)(o[1] >> 11);
    return ((double)w + 0.5) * 1.1102230246251565e-16;
}

// expected count lam = (voxel_vol nbar) (1 + delta_h), delta_h = bias delta or, log-normal, exp(bias delta - s) / mean - 1 with
// mean = sum / n (ln_stats = [s, sum]).  Negative lam -> 0 unless log-normal, NaN -> 0.  COUNTS: the Poisson draw (as T) instead
// of lam.  flag[0] |= 1 where lam > 2^24 (or +inf).
template <typename T, bool COUNTS>
__global__ __launch_bounds__(256) void k_halo_lambda(const T* dx, HPrm nbar, HPrm bias, double vv, int lognormal,
                                                     const double* ln_stats, unsigned long long n, int N, double* lam_out,
                                                     T* counts_out, fb::RngKey key, unsigned* flag) {
    const double ls = lognormal ? ln_stats[0] : 0.0;
    const double mean = lognormal ? ln_stats[1] / (double)n : 1.0;
    bool any_over = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int iz = (int)(i % (unsigned)N);
        double dh = __dmul_rn(hprm_at<T>(bias, i, iz), (double)dx[i]);
        if (lognormal) dh = __dadd_rn(__ddiv_rn(exp(__dadd_rn(dh, -ls)), mean), -1.0);
        double lam = __dmul_rn(__dmul_rn(vv, hprm_at<T>(nbar, i, iz)), __dadd_rn(1.0, dh));
        if (!lognormal && lam < 0.0) lam = 0.0;
        if (lam != lam) lam = 0.0;
        const bool over = lam > FB_HALO_LAM_MAX;
        any_over |= over;
        if (COUNTS) counts_out[i] = (T)(over ? 0.0 : poisson_inverse(lam, poisson_uniform(i, key)));
        else lam_out[i] = lam;
    }
    if (__any(any_over) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- catalogue --------------------------------------------------------------------------------------------------------
// per-workgroup [max count, sum of counts, bad] (bad: a value that is negative, not an integer or not finite)
template <typename T>
__global__ __launch_bounds__(256) void k_cat_stats(const T* counts, unsigned long long n, unsigned long long* partials) {
    double mx = 0.0, sum = 0.0, bad = 0.0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double c = (double)counts[i];
        if (!(c >= 0.0) || c != floor(c) || c > 9.0e15) { bad = 1.0; continue; }
        mx = fmax(mx, c); sum += c;                // integers below 2^53 per lane
    }
    mx = block_reduce(mx, 1);
    bad = block_reduce(bad, 1);
    // exact integer sum: lane sums are integers < 2^53; add them as integers
    __shared__ unsigned long long tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    atomicAdd(&tot, (unsigned long long)sum);
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x] = (unsigned long long)mx;
        partials[3 * blockIdx.x + 1] = tot;
        partials[3 * blockIdx.x + 2] = bad > 0.0 ? 1ull : 0ull;
    }
}
__global__ __launch_bounds__(256) void k_cat_stats_finish(const unsigned long long* partials, int nb, unsigned long long* out) {
    __shared__ unsigned long long r[3];
    if (threadIdx.x < 3) r[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        atomicMax(&r[0], partials[3 * i]);
        atomicAdd(&r[1], partials[3 * i + 1]);
        atomicOr(&r[2], partials[3 * i + 2]);
    }
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = r[threadIdx.x];
}

// H[c nb + b] = voxels of count c in tile b (tile = `tile` consecutive voxels in C order): an LDS histogram of the counts below
// 4096, global atomics for the (rare) larger ones -- integer adds, so the result does not depend on their order
#define FB_CAT_LDS 4096
template <typename T>
__global__ __launch_bounds__(256) void k_cat_hist(const T* counts, unsigned long long n, unsigned long long tile, int nb,
                                                  int kmax, unsigned* H) {
    __shared__ unsigned h[FB_CAT_LDS];
    const unsigned long long b0 = (unsigned long long)blockIdx.x * tile;
    const unsigned long long b1 = b0 + tile < n ? b0 + tile : n;
    const int kl = kmax < FB_CAT_LDS - 1 ? kmax : FB_CAT_LDS - 1;
    for (int c = threadIdx.x; c <= kl; c += 256) h[c] = 0;
    __syncthreads();
    for (unsigned long long i = b0 + threadIdx.x; i < b1; i += 256) {
        const int c = (int)counts[i];
        if (c < 1) continue;
        if (c < FB_CAT_LDS) atomicAdd(&h[c], 1u);
        else atomicAdd(&H[(unsigned long long)c * nb + blockIdx.x], 1u);
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= kl; c += 256) H[(unsigned long long)c * nb + blockIdx.x] = h[c];
}

// the catalogue's scan (fb_scan.h): S[j] = sum_{j' < j} c(j') H[j'], c(j) = j / nb the count of table entry j
struct CatTerm {
    const unsigned* H; int nb;
    __device__ unsigned long long operator()(unsigned long long j) const { return (unsigned long long)(j / (unsigned)nb) * H[j]; }
};

// Emit: workgroup b walks its tile 256 voxels at a time, in order.  A voxel of count c >= 1 is the r-th voxel of that count in
// this step, so its halos start at S[c nb + b] + c r (S is this workgroup's cursor of count c: advanced by c per voxel, by the
// last voxel of each count in the step).  Halo h of voxel (i0, i1, i2): pos[h][a] = (i_a + u) * h_a.
// scatter 0: u = 0; 1: u = U[3 h + a] (uploaded); 2: u = (1 - 1e-8) w_a 2^-32, words of Philox call h of stream 6.
template <typename T>
__global__ __launch_bounds__(256) void k_cat_emit(const T* counts, unsigned long long n, unsigned long long tile, int nb, int N,
                                                  unsigned long long* S, const double* U, int scatter, fb::RngKey key,
                                                  double h0, double h1, double h2, double* pos) {
    __shared__ int sc[256];
    const unsigned long long b0 = (unsigned long long)blockIdx.x * tile;
    const unsigned long long b1 = b0 + tile < n ? b0 + tile : n;
    const unsigned long long NN = (unsigned long long)N * N;
    for (unsigned long long s0 = b0; s0 < b1; s0 += 256) {
        const unsigned long long i = s0 + threadIdx.x;
        const int c = i < b1 ? (int)counts[i] : 0;
        sc[threadIdx.x] = c;
        __syncthreads();
        int rank = 0, tot = 0;
        if (c >= 1)
            for (int t = 0; t < 256; ++t) {
                const int e = sc[t] == c;
                tot += e;
                rank += e & (t < (int)threadIdx.x);
            }
        unsigned long long base = 0;
        unsigned long long* cur = c >= 1 ? S + (unsigned long long)c * nb + blockIdx.x : nullptr;
        if (c >= 1) base = *cur;
        __syncthreads();
        if (c >= 1 && rank + 1 == tot) *cur = base + (unsigned long long)c * tot;
        if (c >= 1) {
            const double x0 = (double)(i / NN), x1 = (double)((i / (unsigned)N) % (unsigned)N), x2 = (double)(i % (unsigned)N);
            unsigned long long hk = base + (unsigned long long)c * rank;
            for (int k = 0; k < c; ++k, ++hk) {
                double u0 = 0.0, u1 = 0.0, u2 = 0.0;
                if (scatter == 1) { u0 = U[3 * hk]; u1 = U[3 * hk + 1]; u2 = U[3 * hk + 2]; }
                else if (scatter == 2) {
                    uint32_t o[4];
                    fb::philox4x32(hk, 6u, key, o);
                    u0 = (1.0 - 1e-8) * ((double)o[0] * 2.3283064365386963e-10);
                    u1 = (1.0 - 1e-8) * ((double)o[1] * 2.3283064365386963e-10);
                    u2 = (1.0 - 1e-8) * ((double)o[2] * 2.3283064365386963e-10);
                }
                pos[3 * hk] = __dmul_rn(__dadd_rn(x0, u0), h0);
                pos[3 * hk + 1] = __dmul_rn(__dadd_rn(x1, u1), h1);
                pos[3 * hk + 2] = __dmul_rn(__dadd_rn(x2, u2), h2);
            }
        }
        __syncthreads();
    }
}

// ---- painting -----------------------------------------------------------------------------------------------------------
// Fixed point: every contribution x = w W is added as the integer round(x 2^F) -- order-independent, so the mesh is the same
// bit for bit from call to call.  F = 61 - e with sum |w| < 2^e, so no node can overflow 62 bits.  TWO (fp64 plans): v = x 2^F'
// with F' = F + 32 is split into hi = floor(v 2^-32) (int64) and lo = v - hi 2^32 in [0, 2^32], two accumulators: about 94
// significant bits per node.  k_paint_wsum<> and k_paint_finish<> live in fb_dev.h: fb_regrid.hip's histogram shares them.
// (axis_weights, the nodes and weights of one axis, lives in fb_dev.h: fb_recon.hip reads the mesh back through them)
template <bool TWO>
__global__ __launch_bounds__(256) void k_paint(const double* pos, const double* wt, unsigned long long n, int window, int N,
                                               double s0, double s1, double s2, const double* wsum,
                                               unsigned long long* acc_hi, unsigned long long* acc_lo) {
    const int F = fx_exponent(wsum[0], 61) + (TWO ? 32 : 0);
    const double scale = ldexp(1.0, F);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double x0 = pos[3 * i], x1 = pos[3 * i + 1], x2 = pos[3 * i + 2];
        if (!(fabs(x0) < 1e300 && fabs(x1) < 1e300 && fabs(x2) < 1e300)) continue;      // not finite: nothing to add
        const double wi = wt ? wt[i] : 1.0;
        long long m0[3], m1[3], m2[3];
        double w0[3], w1[3], w2[3];
        const int n0 = axis_weights(x0 * s0, window, N, m0, w0);
        const int n1 = axis_weights(x1 * s1, window, N, m1, w1);
        const int n2 = axis_weights(x2 * s2, window, N, m2, w2);
        for (int a = 0; a < n0; ++a)
            for (int b = 0; b < n1; ++b) {
                const unsigned long long row = ((unsigned long long)m0[a] * N + (unsigned long long)m1[b]) * N;
                const double wab = (wi * w0[a]) * w1[b];
                for (int c = 0; c < n2; ++c) {
                    const double v = (wab * w2[c]) * scale;
                    if (TWO) {
                        unsigned long long hi, lo;
                        fx_split(v, hi, lo);
                        atomicAdd(&acc_hi[row + m2[c]], hi);
                        atomicAdd(&acc_lo[row + m2[c]], lo);
                    } else {
                        atomicAdd(&acc_hi[row + m2[c]], (unsigned long long)__double2ll_rn(v));
                    }
                }
            }
    }
}
// compensation: every stored mode of a half spectrum divided by prod_a sinc(pi m_a / N)^p, then the c2r's 1/N^3
template <typename T>
__global__ __launch_bounds__(256) void k_paint_compensate(T* half, int N, int NR, int NZP, int p) {
    const int NZV = N / 2 + 1;
    const unsigned long long n = (unsigned long long)N * NR * NZP;
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256) {
        const unsigned long long row = q / (unsigned)NZP;
        const int l = (int)(q - row * (unsigned)NZP), j = (int)(row % (unsigned)NR), i = (int)(row / (unsigned)NR);
        if (l >= NZV || j >= N) continue;
        const int ms[3] = {i <= N / 2 ? i : i - N, j <= N / 2 ? j : j - N, l};     // (N/2 stays +N/2: not mode_of; sinc is even)
        double f = 1.0;
        for (int a = 0; a < 3; ++a) {
            if (!ms[a]) continue;
            const double x = 3.14159265358979323846 * (double)ms[a] / (double)N;
            const double sc = sin(x) / x;
            double t = sc;
            for (int k = 1; k < p; ++k) t *= sc;
            f *= t;
        }
        half[2 * q] = (T)((double)half[2 * q] / f);              // (re, im) pairs
        half[2 * q + 1] = (T)((double)half[2 * q + 1] / f);
    }
}

fb::RngKey rng_key(uint64_t seed, uint64_t real) {
    fb::RngKey k;
    k.k[0] = (uint32_t)seed; k.k[1] = (uint32_t)(seed >> 32); k.k[2] = (uint32_t)real; k.k[3] = (uint32_t)(real >> 32);
    return k;
}
int prm_check(const fb_plan* p, const void* ptr, int kind) {
    FB_REQUIRE(kind >= FB_HALO_SCALAR && kind <= FB_HALO_FIELD_F64, "nbar / bias kind must be FB_HALO_SCALAR .. FB_HALO_FIELD_F64");
    FB_REQUIRE(kind == FB_HALO_SCALAR || ptr, "nbar / bias: null device pointer");
    (void)p;
    return FB_OK;
}

// lam (COUNTS false, into lam_out) or the Poisson counts (COUNTS true, into counts_out); flag (device) |= 1 where lam > 2^24
template <typename T, bool COUNTS>
int halo_lambda(fb_plan* p, const void* delta, HPrm nbar, HPrm bias, double vv, int lognormal, double* lam_out, void* counts_out,
                uint64_t seed, uint64_t real, hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->N * p->N;
    int r = p->halo_small.ensure(FB_HALO_SMALL);
    if (r) return r;
    double* part = p->halo_small.as<double>();           // [FB_HALO_RED_BLOCKS] partials
    double* stats = part + FB_HALO_RED_BLOCKS;           // [shift, sum]
    unsigned* flag = (unsigned*)(stats + 2);
    FB_HIP(hipMemsetAsync(flag, 0, sizeof(unsigned), s));
    if (lognormal) {
        const int nb = std::min(grid_for(n, p), FB_HALO_RED_BLOCKS);
        if (sizeof(T) == 4) {          // shift by the maximum (single-precision plans; fp64 plans follow the reference: no shift)
            hipLaunchKernelGGL((k_halo_ln_reduce<T>), dim3(nb), dim3(256), 0, s, (const T*)delta, bias, n, p->N, 1, stats, part);
            FB_LAUNCH_CHECK("k_halo_ln_reduce");
            hipLaunchKernelGGL(k_halo_finish<>, dim3(1), dim3(256), 0, s, part, nb, 1, stats);
            FB_LAUNCH_CHECK("k_halo_finish");
        } else {
            FB_HIP(hipMemsetAsync(stats, 0, sizeof(double), s));
        }
        hipLaunchKernelGGL((k_halo_ln_reduce<T>), dim3(nb), dim3(256), 0, s, (const T*)delta, bias, n, p->N, 0, stats, part);
        FB_LAUNCH_CHECK("k_halo_ln_reduce");
        hipLaunchKernelGGL(k_halo_finish<>, dim3(1), dim3(256), 0, s, part, nb, 0, stats + 1);
        FB_LAUNCH_CHECK("k_halo_finish");
    }
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_halo_lambda<T, COUNTS>), dim3(grid_for(n, p)), dim3(256), 0, s, (const T*)delta, nbar, bias, vv, lognormal,
                       (const double*)stats, n, p->N, lam_out, (T*)counts_out, rng_key(seed, real), flag); }
    FB_LAUNCH_CHECK("k_halo_lambda");
    return FB_OK;
}

template <typename T>
int cat_stats(fb_plan* p, const void* counts, int64_t* out_host, hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->N * p->N;
    int r = p->halo_small.ensure(FB_HALO_SMALL);
    if (r) return r;
    unsigned long long* part = p->halo_small.as<unsigned long long>();
    const int nb = std::min(grid_for(n, p), FB_HALO_RED_BLOCKS - 2);
    unsigned long long* res = part + 3 * (FB_HALO_RED_BLOCKS - 2);
    hipLaunchKernelGGL((k_cat_stats<T>), dim3(nb), dim3(256), 0, s, (const T*)counts, n, part);
    FB_LAUNCH_CHECK("k_cat_stats");
    hipLaunchKernelGGL(k_cat_stats_finish, dim3(1), dim3(256), 0, s, (const unsigned long long*)part, nb, res);
    FB_LAUNCH_CHECK("k_cat_stats_finish");
    unsigned long long h[3];
    FB_TRY(fb_read_back(h, res, sizeof(h), s));
    FB_REQUIRE(!h[2], "halo counts must be non-negative integers");
    out_host[0] = (int64_t)h[0];
    out_host[1] = (int64_t)h[1];
    return FB_OK;
}

template <typename T>
int cat_emit(fb_plan* p, const void* counts, int64_t kmax, const double* U, int scatter, uint64_t seed, uint64_t real, double* pos,
             hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->N * p->N;
    const unsigned long long K = (unsigned long long)kmax + 1;
    // tiles: at least FB_HALO_TILE_MIN voxels, and no more (count, tile) entries than FB_HALO_TABLE_MAX
    unsigned long long tile = FB_HALO_TILE_MIN;
    while ((n + tile - 1) / tile * K > FB_HALO_TABLE_MAX && tile < n) tile *= 2;
    const int nb = (int)((n + tile - 1) / tile);
    const unsigned long long M = K * nb;
    // work: H [M] u32 | S [M + 1] u64 (S[M]: the total, not read) | csum [chunks] u64
    const size_t offS = (M * 4 + 15) / 16 * 16, offC = offS + (M + 1) * 8;
    int r = p->halo_work.ensure(offC + (size_t)scan_chunks(M) * 8);
    if (r) return r;
    unsigned* H = p->halo_work.as<unsigned>();
    unsigned long long* S = (unsigned long long*)(p->halo_work.as<char>() + offS);
    unsigned long long* csum = (unsigned long long*)(p->halo_work.as<char>() + offC);
    FB_HIP(hipMemsetAsync(H, 0, M * 4, s));
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cat_hist<T>), dim3(nb), dim3(256), 0, s, (const T*)counts, n, tile, nb, (int)kmax, H); }
    FB_LAUNCH_CHECK("k_cat_hist");
    r = exscan(CatTerm{H, nb}, M, csum, S, s);
    if (r) return r;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cat_emit<T>), dim3(nb), dim3(256), 0, s, (const T*)counts, n, tile, nb, p->N, S, U, scatter,
                       rng_key(seed, real), p->L[0] / (double)p->N, p->L[1] / (double)p->N, p->L[2] / (double)p->N, pos); }
    FB_LAUNCH_CHECK("k_cat_emit");
    return FB_OK;
}

template <typename T>
int paint(fb_plan* p, const double* pos, const double* wt, unsigned long long n, int window, void* out, hipStream_t s) {
    const unsigned long long nv = (unsigned long long)p->N * p->N * p->N;
    constexpr bool TWO = sizeof(T) == 8;
    int r = p->halo_small.ensure(FB_HALO_SMALL);
    if (!r) r = p->halo_acc.ensure(nv * 8 * (TWO ? 2 : 1));
    if (r) return r;
    double* part = p->halo_small.as<double>();
    double* wsum = part + FB_HALO_RED_BLOCKS;
    unsigned long long* hi = p->halo_acc.as<unsigned long long>();
    unsigned long long* lo = TWO ? hi + nv : nullptr;
    FB_HIP(hipMemsetAsync(hi, 0, nv * 8 * (TWO ? 2 : 1), s));
    const int nb = std::min(grid_for(n, p), FB_HALO_RED_BLOCKS);
    hipLaunchKernelGGL(k_paint_wsum<>, dim3(nb), dim3(256), 0, s, wt, n, part);
    FB_LAUNCH_CHECK("k_paint_wsum");
    hipLaunchKernelGGL(k_halo_finish<>, dim3(1), dim3(256), 0, s, (const double*)part, nb, 0, wsum);
    FB_LAUNCH_CHECK("k_halo_finish");
    if (n) {
        FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL((k_paint<TWO>), dim3(grid_for(n, p)), dim3(256), 0, s, pos, wt, n, window, p->N,
                           (double)p->N / p->L[0], (double)p->N / p->L[1], (double)p->N / p->L[2], (const double*)wsum, hi, lo);
    }
    FB_LAUNCH_CHECK("k_paint");
    hipLaunchKernelGGL((k_paint_finish<T, TWO>), dim3(grid_for(nv, p)), dim3(256), 0, s, (const unsigned long long*)hi,
                       (const unsigned long long*)lo, nv, (const double*)wsum, (T*)out);
    FB_LAUNCH_CHECK("k_paint_finish");
    return FB_OK;
}

template <typename T>
int compensate(fb_plan* p, void* half, int pw, hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->NR * p->NZP;
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_paint_compensate<T>), dim3(grid_for(n, p)), dim3(256), 0, s, (T*)half, p->N, p->NR, p->NZP, pw); }
    FB_LAUNCH_CHECK("k_paint_compensate");
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_halo_lambda(fb_plan* p, const void* delta, const void* nbar, int nbar_kind, double nbar_val, const void* bias, int bias_kind,
                   double bias_val, double voxel_vol, int lognormal, double* lam_out, void* stream) {
    FB_REQUIRE(p && delta && lam_out, "null pointer");
    int r = prm_check(p, nbar, nbar_kind);
    if (!r) r = prm_check(p, bias, bias_kind);
    if (r) return r;
    FB_USE_DEVICE(p);
    const HPrm nb{nbar, nbar_val, nbar_kind}, bs{bias, bias_val, bias_kind};
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, (halo_lambda<float, false>(p, delta, nb, bs, voxel_vol, lognormal, lam_out, nullptr, 0, 0, s)),
                       (halo_lambda<double, false>(p, delta, nb, bs, voxel_vol, lognormal, lam_out, nullptr, 0, 0, s)));
}

int fb_halo_counts(fb_plan* p, const void* delta, const void* nbar, int nbar_kind, double nbar_val, const void* bias, int bias_kind,
                   double bias_val, double voxel_vol, int lognormal, uint64_t seed, uint64_t realisation, void* counts_out,
                   int* too_large, void* stream) {
    FB_REQUIRE(p && delta && counts_out && too_large, "null pointer");
    int r = prm_check(p, nbar, nbar_kind);
    if (!r) r = prm_check(p, bias, bias_kind);
    if (r) return r;
    FB_USE_DEVICE(p);
    const HPrm nb{nbar, nbar_val, nbar_kind}, bs{bias, bias_val, bias_kind};
    hipStream_t s = (hipStream_t)stream;
    r = FB_DISPATCH(p, (halo_lambda<float, true>(p, delta, nb, bs, voxel_vol, lognormal, nullptr, counts_out, seed, realisation, s)),
                    (halo_lambda<double, true>(p, delta, nb, bs, voxel_vol, lognormal, nullptr, counts_out, seed, realisation, s)));
    if (r) return r;
    unsigned flag = 0;
    const unsigned* fdev = (const unsigned*)(p->halo_small.as<double>() + FB_HALO_RED_BLOCKS + 2);
    FB_TRY(fb_read_back(&flag, fdev, sizeof(flag), s));
    *too_large = flag ? 1 : 0;
    return FB_OK;
}

int fb_halo_catalogue_size(fb_plan* p, const void* counts, int64_t* kmax_total, void* stream) {
    FB_REQUIRE(p && counts && kmax_total, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, cat_stats<float>(p, counts, kmax_total, s), cat_stats<double>(p, counts, kmax_total, s));
}

int fb_halo_catalogue(fb_plan* p, const void* counts, int64_t kmax, int64_t total, const double* uniforms, int scatter,
                      uint64_t seed, uint64_t realisation, double* pos_out, void* stream) {
    FB_REQUIRE(p && counts, "null pointer");
    FB_REQUIRE(kmax >= 0 && kmax <= (int64_t)FB_HALO_LAM_MAX * 4 && total >= 0, "kmax / total out of range");
    FB_REQUIRE(scatter >= 0 && scatter <= 2, "scatter must be 0, 1 or 2");
    FB_REQUIRE(scatter != 1 || uniforms, "scatter 1 needs the uniforms");
    if (total == 0) return FB_OK;
    FB_REQUIRE(pos_out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, cat_emit<float>(p, counts, kmax, uniforms, scatter, seed, realisation, pos_out, s),
                       cat_emit<double>(p, counts, kmax, uniforms, scatter, seed, realisation, pos_out, s));
}

int fb_paint(fb_plan* p, const double* pos, const double* weights, int64_t n, int window, void* real_out, void* stream) {
    FB_REQUIRE(p && real_out && (pos || n == 0), "null pointer");
    FB_REQUIRE(n >= 0, "n must be >= 0");
    FB_REQUIRE(window >= FB_WINDOW_NGP && window <= FB_WINDOW_TSC, "window must be FB_WINDOW_NGP, _CIC or _TSC");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, paint<float>(p, pos, weights, (unsigned long long)n, window, real_out, s),
                       paint<double>(p, pos, weights, (unsigned long long)n, window, real_out, s));
}

int fb_paint_compensate(fb_plan* p, void* real_inout, void* work_half, int window, void* stream) {
    FB_REQUIRE(p && real_inout && work_half, "null pointer");
    FB_REQUIRE(window >= FB_WINDOW_NGP && window <= FB_WINDOW_TSC, "window must be FB_WINDOW_NGP, _CIC or _TSC");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const double n3 = (double)p->N * p->N * p->N;
    int r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real_inout, work_half, 0, s), fbi_fft_r2c_f64(p, real_inout, work_half, 0, s));
    if (!r) r = FB_DISPATCH(p, compensate<float>(p, work_half, window + 1, s), compensate<double>(p, work_half, window + 1, s));
    if (!r) r = FB_DISPATCH(p, fbi_fft_c2r_f32(p, work_half, real_inout, 1.0 / n3, s), fbi_fft_c2r_f64(p, work_half, real_inout, 1.0 / n3, s));
    return r;
}

}  // extern "C"
