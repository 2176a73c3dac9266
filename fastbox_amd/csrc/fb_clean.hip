// Foreground cleaning beyond PCA (the reference's fastbox/filters.py:187-243, :373-491): the coordinate-descent sweep of
// non-negative matrix factorisation, the fixed-point step of FastICA, and the small helpers their drivers in
// fastbox_amd/filters.py need.  Both plan precisions are compiled here; every sum is formed in fp64 in a fixed order (per
// workgroup partials, then one finishing kernel): no floating-point atomics, results are bitwise repeatable.  Definitions:
// DESIGN.md section 4; entry points: include/fastbox_hip.h.
//
// The cube is T[pixel = (x, y)][channel], the channel contiguous.  W[k][npix] and X1[n][npix] are fp64 in the layout of
// fb_pca_clean's amps_dev; H[k][N] is fp64, one component's spectrum contiguous.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <cmath>

#define FB_CLEAN_KMAX 16                 // components (NMF) / sources (ICA)
#define FB_CLEAN_NMAX 1024               // channels of the NMF sweep: four spectra in fp64 take 32 KiB of LDS
#define FB_CLEAN_RED_BLOCKS 1024         // workgroups of the grid-stride reductions (and the most of fb_ica_step_split)

namespace {
using namespace fb;
static_assert(FB_CLEAN_RED_BLOCKS == 1024, "fb_ica_step_split (fb_plan.h) caps the workgroups of k_ica_step at 1024");

// One cyclic coordinate-descent pass over the k coefficients v[] of one row (scikit-learn's _update_cdnmf_fast, no
// regularisation, no shuffling): b[t] = the row of X H^T (or X^T W), A = H H^T (or W^T W), k x k in LDS.
// Returns the row's share of the projected-gradient violation.
__device__ __forceinline__ double cd_row(double (&v)[FB_CLEAN_KMAX], const double (&b)[FB_CLEAN_KMAX], const double* A, int k) {
    double viol = 0.0;
#pragma unroll
    for (int t = 0; t < FB_CLEAN_KMAX; ++t) {
        if (t < k) {
            double grad = -b[t];
#pragma unroll
            for (int r = 0; r < FB_CLEAN_KMAX; ++r) if (r < k) grad += A[t * k + r] * v[r];
            const double pg = v[t] == 0.0 ? fmin(0.0, grad) : grad;
            viol += fabs(pg);
            const double hess = A[t * k + t];
            if (hess != 0.0) v[t] = fmax(v[t] - grad / hess, 0.0);
        }
    }
    return viol;
}

// A[t][r] = sum_c M[t][c] M[r][c] (H H^T): one workgroup, thread (t, r), channels in ascending order
__global__ __launch_bounds__(256) void k_nmf_gram(const double* __restrict__ M, int k, int N, double* __restrict__ A) {
    const int t = threadIdx.x >> 4, r = threadIdx.x & 15;
    if (t >= k || r >= k) return;
    double s = 0.0;
    for (int c = 0; c < N; ++c) s += M[(size_t)t * N + c] * M[(size_t)r * N + c];
    A[t * k + r] = s;
}

// The W half of one NMF iteration in one pass over the cube.  A workgroup of four waves walks its share of the pixels four
// at a time.  Each wave holds one pixel's spectrum in registers (lane l: channels l, l + 64, ...), forms its k entries of
// X H^T (H from global memory: k N doubles, cache resident), sweeps the W row and stores it.  The four spectra and W rows
// then meet in LDS, and the workgroup adds them, in pixel order, to its partial sums: wave w owns components w, w + 4, ... of
// X^T W for every channel (CPL x 4 accumulators per lane), thread (t, r) one entry of W^T W.  A slot past the last pixel holds
// zeros.  partial[workgroup] = [X^T W: N k | W^T W: k k | violation].
template <typename T, int CPL>
__global__ __launch_bounds__(256) void k_nmf_sweep(const T* __restrict__ cube, double* __restrict__ W, const double* __restrict__ H,
                                                   const double* __restrict__ HHt, int k, long long npix, int N,
                                                   long long per, double* __restrict__ partial) {
    extern __shared__ double lds[];
    double* A = lds;                                  // [k][k]
    double* ws = lds + FB_CLEAN_KMAX * FB_CLEAN_KMAX; // [4][16]
    double* xs = ws + 4 * FB_CLEAN_KMAX;              // [4][N]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)threadIdx.x < k * k) A[threadIdx.x] = HHt[threadIdx.x];
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;     // per: fb_nmf_sweep_split
    double acc[CPL][4];
#pragma unroll
    for (int q = 0; q < CPL; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[q][j] = 0.0;
    double aww = 0.0, viol = 0.0;
    const int wt = threadIdx.x >> 4, wr = threadIdx.x & 15;
    for (long long pb = p0; pb < p1; pb += 4) {
        const long long p = pb + wave;
        const bool live = p < p1;
        double x[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = lane + 64 * q;
            x[q] = (live && c < N) ? (double)cube[p * N + c] : 0.0;
        }
        double w[FB_CLEAN_KMAX], b[FB_CLEAN_KMAX];
#pragma unroll
        for (int t = 0; t < FB_CLEAN_KMAX; ++t) {
            w[t] = 0.0; b[t] = 0.0;
            if (t < k) {
                double a = 0.0;
#pragma unroll
                for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) a += H[(size_t)t * N + c] * x[q]; }
                b[t] = wave_sum(a);
                if (live) w[t] = W[(size_t)t * npix + p];
            }
        }
        if (live) {
            const double v = cd_row(w, b, A, k);
            if (lane == 0) viol += v;
        }
#pragma unroll
        for (int t = 0; t < FB_CLEAN_KMAX; ++t) {
            if (t < k && lane == t) {
                if (live) W[(size_t)t * npix + p] = w[t];
                ws[wave * FB_CLEAN_KMAX + t] = w[t];
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) xs[wave * N + c] = x[q]; }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = wave + 4 * j;
                if (t < k) {
                    const double wv = ws[s * FB_CLEAN_KMAX + t];
#pragma unroll
                    for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) acc[q][j] += wv * xs[s * N + c]; }
                }
            }
            if (wt < k && wr < k) aww += ws[s * FB_CLEAN_KMAX + wt] * ws[s * FB_CLEAN_KMAX + wr];
        }
        __syncthreads();
    }
    const size_t m = (size_t)N * k + (size_t)k * k + 1;
    double* dst = partial + (size_t)blockIdx.x * m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = wave + 4 * j;
        if (t < k) {
#pragma unroll
            for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) dst[(size_t)c * k + t] = acc[q][j]; }
        }
    }
    if (wt < k && wr < k) dst[(size_t)N * k + wt * k + wr] = aww;
    if (lane == 0) ws[wave] = viol;
    __syncthreads();
    if (threadIdx.x == 0) dst[m - 1] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// out[i] = scale * sum over the workgroups' partials, in workgroup order (four interleaved chains)
__global__ __launch_bounds__(256) void k_sum_rows(const double* __restrict__ partial, int nb, long long m, double scale,
                                                  double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int b = 0;
    for (; b + 3 < nb; b += 4) {
        a0 += partial[(size_t)b * m + i]; a1 += partial[(size_t)(b + 1) * m + i];
        a2 += partial[(size_t)(b + 2) * m + i]; a3 += partial[(size_t)(b + 3) * m + i];
    }
    for (; b < nb; ++b) a0 += partial[(size_t)b * m + i];
    out[i] = ((a0 + a1) + (a2 + a3)) * scale;
}

// The H half: the same sweep on the rows of H^T with A = W^T W and b = X^T W (both from `sums`, the finished partials of
// k_nmf_sweep).  One workgroup, a thread per channel; viol[0] = the W half's violation, viol[1] = this half's.
__global__ __launch_bounds__(256) void k_nmf_update_h(double* __restrict__ H, const double* __restrict__ sums, int k, int N,
                                                      double* __restrict__ viol) {
    __shared__ double A[FB_CLEAN_KMAX * FB_CLEAN_KMAX];
    __shared__ double red[256];
    if ((int)threadIdx.x < k * k) A[threadIdx.x] = sums[(size_t)N * k + threadIdx.x];
    __syncthreads();
    double vsum = 0.0;
    for (int c = threadIdx.x; c < N; c += 256) {
        double h[FB_CLEAN_KMAX], b[FB_CLEAN_KMAX];
#pragma unroll
        for (int t = 0; t < FB_CLEAN_KMAX; ++t) {
            h[t] = t < k ? H[(size_t)t * N + c] : 0.0;
            b[t] = t < k ? sums[(size_t)c * k + t] : 0.0;
        }
        vsum += cd_row(h, b, A, k);
#pragma unroll
        for (int t = 0; t < FB_CLEAN_KMAX; ++t) if (t < k) H[(size_t)t * N + c] = h[t];
    }
    red[threadIdx.x] = vsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += red[i];
        viol[0] = sums[(size_t)N * k + (size_t)k * k];
        viol[1] = s;
    }
}

// out[p][c] = x[p][c] - sum_t W[t][p] H[t][c]; partial[workgroup] = sum of the squared residuals (fp64, before rounding
// to T).  One wave per pixel at a time, workgroups stride over the pixels.  out may be null (the norm only).
template <typename T, int CPL>
__global__ __launch_bounds__(256) void k_nmf_residual(const T* __restrict__ cube, const double* __restrict__ W,
                                                      const double* __restrict__ H, int k, long long npix, int N,
                                                      T* __restrict__ out, double* __restrict__ partial) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double ss = 0.0;
    for (long long p = (long long)blockIdx.x * 4 + wave; p < npix; p += (long long)gridDim.x * 4) {
        double r[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; r[q] = c < N ? (double)cube[p * N + c] : 0.0; }
        for (int t = 0; t < k; ++t) {
            const double wv = W[(size_t)t * npix + p];
#pragma unroll
            for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) r[q] -= wv * H[(size_t)t * N + c]; }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = lane + 64 * q;
            if (c < N) { ss += r[q] * r[q]; if (out) out[p * N + c] = (T)r[q]; }
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// NNDSVD on the rows of a[k][npix] (U S of the leading singular triplets): partial[workgroup][2 j], [2 j + 1] = the sums
// of squares of the positive and of the negative entries of row j over the workgroup's pixels
__global__ __launch_bounds__(256) void k_rows_posneg(const double* __restrict__ a, int k, long long npix, double* __restrict__ partial) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j < k; ++j) {
        double sp = 0.0, sn = 0.0;
        for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
            const double v = a[(size_t)j * npix + p];
            if (v > 0.0) sp += v * v; else sn += v * v;
        }
        sp = wave_sum(sp); sn = wave_sum(sn);
        if (lane == 0) { red[wave][0] = sp; red[wave][1] = sn; }
        __syncthreads();
        if (threadIdx.x < 2)
            partial[(size_t)blockIdx.x * 2 * k + 2 * j + threadIdx.x] =
                (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        __syncthreads();
    }
}
// a[j][p] <- max(coef[j] a[j][p], 0) (row 0 with abs_first: |coef[0] a[0][p]|), then values below eps become `fill`
__global__ __launch_bounds__(256) void k_rows_rectify(double* __restrict__ a, int k, long long npix, const double* __restrict__ coef,
                                                      int abs_first, double eps, double fill) {
    const long long n = (long long)k * npix;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / npix);
        double v = coef[j] * a[i];
        v = (j == 0 && abs_first) ? fabs(v) : fmax(v, 0.0);
        a[i] = v < eps ? fill : v;
    }
}

// partial[workgroup] = (least value, number of values that are not finite); NaN never wins the comparison
template <typename T>
__global__ __launch_bounds__(256) void k_min_finite(const T* __restrict__ x, long long n, double* __restrict__ partial) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mn = INFINITY, bad = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = (double)x[i];
        if (!isfinite(v)) bad += 1.0;
        if (v < mn) mn = v;
    }
    mn = wave_min_cmp(mn);
    bad = wave_sum(bad);
    if (lane == 0) { red[wave][0] = mn; red[wave][1] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0][0], b = red[0][1];
        for (int w = 1; w < 4; ++w) { m = red[w][0] < m ? red[w][0] : m; b += red[w][1]; }
        partial[2 * blockIdx.x] = m; partial[2 * blockIdx.x + 1] = b;
    }
}
__global__ void k_min_finish(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    double m = partial[0], b = partial[1];
    for (int i = 1; i < nb; ++i) { m = partial[2 * i] < m ? partial[2 * i] : m; b += partial[2 * i + 1]; }
    out[0] = m; out[1] = b;
}

// real part of a complex cube
template <typename T>
__global__ __launch_bounds__(256) void k_real_part(const T* __restrict__ in, T* __restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = in[2 * i];
}

// ---- FastICA ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ica_g(int fun, double alpha, double y, double& g, double& gp) {
    if (fun == FB_ICA_LOGCOSH) { const double th = tanh(alpha * y); g = th; gp = alpha * (1.0 - th * th); }
    else if (fun == FB_ICA_EXP) { const double e = exp(-(y * y) / 2.0); g = y * e; gp = (1.0 - y * y) * e; }
    else { g = y * y * y; gp = 3.0 * y * y; }
}
// One fixed-point step's sums: partial[workgroup] = [sum_p g(y_i) x_j : n n | sum_p g'(y_i) : n], y = Wm x, x = X1[:, p].
// Thread (i = tid / 16, l = tid % 16) takes row i for the pixels l, l + 16, ... of the workgroup's share, with the pixel's
// n-vector in registers: n + 1 accumulators per thread instead of n^2 + n.  The 16 pixel lanes of a row are then added in
// lane order through LDS.
__global__ __launch_bounds__(256) void k_ica_step(const double* __restrict__ Wm, const double* __restrict__ X1, int n,
                                                  long long npix, long long per, int fun, double alpha,
                                                  double* __restrict__ partial) {
    __shared__ double sh[16][16][FB_CLEAN_KMAX + 1];
    const int i = threadIdx.x >> 4, l = threadIdx.x & 15;
    const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;     // per: fb_ica_step_split
    double wrow[FB_CLEAN_KMAX], acc[FB_CLEAN_KMAX], agp = 0.0;
#pragma unroll
    for (int j = 0; j < FB_CLEAN_KMAX; ++j) { wrow[j] = (i < n && j < n) ? Wm[i * n + j] : 0.0; acc[j] = 0.0; }
    if (i < n) {
        for (long long p = p0 + l; p < p1; p += 16) {
            double x[FB_CLEAN_KMAX], y = 0.0;
#pragma unroll
            for (int j = 0; j < FB_CLEAN_KMAX; ++j) { x[j] = j < n ? X1[(size_t)j * npix + p] : 0.0; y += wrow[j] * x[j]; }
            double g, gp;
            ica_g(fun, alpha, y, g, gp);
            agp += gp;
#pragma unroll
            for (int j = 0; j < FB_CLEAN_KMAX; ++j) acc[j] += g * x[j];
        }
    }
#pragma unroll
    for (int j = 0; j < FB_CLEAN_KMAX; ++j) sh[i][l][j] = acc[j];
    sh[i][l][FB_CLEAN_KMAX] = agp;
    __syncthreads();
    double* dst = partial + (size_t)blockIdx.x * (n * n + n);
    if (i < n && l < n) {
        double s = 0.0;
        for (int q = 0; q < 16; ++q) s += sh[i][q][l];
        dst[i * n + l] = s;
    }
    if (i < n && l == 15) {
        double s = 0.0;
        for (int q = 0; q < 16; ++q) s += sh[i][q][FB_CLEAN_KMAX];
        dst[n * n + i] = s;
    }
}
// S[i][p] = scale[i] sum_j Wm[i][j] X1[j][p]; partial[workgroup] = [sum_p S_i : n | sum_p S_i^2 : n] (one thread per pixel)
__global__ __launch_bounds__(256) void k_ica_sources(const double* __restrict__ Wm, const double* __restrict__ scale,
                                                     const double* __restrict__ X1, int n, long long npix, double* __restrict__ S,
                                                     double* __restrict__ partial) {
    __shared__ double wl[FB_CLEAN_KMAX * FB_CLEAN_KMAX + FB_CLEAN_KMAX];
    __shared__ double red[4][2 * FB_CLEAN_KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)threadIdx.x < n * n) wl[threadIdx.x] = Wm[threadIdx.x];
    if ((int)threadIdx.x < n) wl[FB_CLEAN_KMAX * FB_CLEAN_KMAX + threadIdx.x] = scale[threadIdx.x];
    __syncthreads();
    double s1[FB_CLEAN_KMAX], s2[FB_CLEAN_KMAX];
#pragma unroll
    for (int i = 0; i < FB_CLEAN_KMAX; ++i) s1[i] = s2[i] = 0.0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
        double x[FB_CLEAN_KMAX];
#pragma unroll
        for (int j = 0; j < FB_CLEAN_KMAX; ++j) x[j] = j < n ? X1[(size_t)j * npix + p] : 0.0;
#pragma unroll
        for (int i = 0; i < FB_CLEAN_KMAX; ++i) {
            if (i < n) {
                double y = 0.0;
#pragma unroll
                for (int j = 0; j < FB_CLEAN_KMAX; ++j) if (j < n) y += wl[i * n + j] * x[j];
                y *= wl[FB_CLEAN_KMAX * FB_CLEAN_KMAX + i];
                S[(size_t)i * npix + p] = y;
                s1[i] += y; s2[i] += y * y;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < FB_CLEAN_KMAX; ++i) {
        if (i < n) {
            const double a = wave_sum(s1[i]), b = wave_sum(s2[i]);
            if (lane == 0) { red[wave][i] = a; red[wave][FB_CLEAN_KMAX + i] = b; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * n) {
        const int i = threadIdx.x % n, which = threadIdx.x / n, o = which * FB_CLEAN_KMAX + i;
        partial[(size_t)blockIdx.x * 2 * n + threadIdx.x] = (red[0][o] + red[1][o]) + (red[2][o] + red[3][o]);
    }
}

// B[p][m] = sum_c Vt[m][c] x[p][c]: every pixel's spectrum in the basis of the N rows of Vt, in fp64.  One wave per pixel, the
// spectrum in registers (lane l: channels l, l + 64, ...); a row of Vt is read along the channels (coalesced, N^2 doubles, cache
// resident), one 64-lane butterfly per coefficient; lane j keeps coefficient m0 + j, so 64 of them leave in one store.
template <typename T, int CPL>
__global__ __launch_bounds__(256) void k_rotate_spectra(const T* __restrict__ cube, const double* __restrict__ Vt,
                                                        double* __restrict__ B, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;                                      // the whole wave
    double x[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; x[q] = c < N ? (double)cube[p * N + c] : 0.0; }
    for (int m0 = 0; m0 < N; m0 += 64) {
        const int mend = N - m0 < 64 ? N - m0 : 64;
        double keep = 0.0;
        for (int j = 0; j < mend; ++j) {
            const double* row = Vt + (size_t)(m0 + j) * N;
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < N) a += row[c] * x[q]; }
            a = wave_sum(a);
            if (lane == j) keep = a;
        }
        if (lane < mend) B[p * N + m0 + lane] = keep;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
int red_blocks(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < FB_CLEAN_RED_BLOCKS ? (b < 1 ? 1 : b) : FB_CLEAN_RED_BLOCKS);
}
int channels_per_lane(int N) {
    int cpl = 1;
    while (64 * cpl < N) cpl *= 2;
    return cpl;
}
void sum_rows(const double* partial, int nb, long long m, double scale, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, partial, nb, m, scale, out);
}

template <typename T>
int nmf_sweep(fb_plan* p, const void* cube, double* W, double* H, int k, double* viol_host, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    if (N > FB_CLEAN_NMAX) { fb_set_error("fb_nmf_sweep: at most 1024 channels"); return FB_ERR_UNSUPPORTED; }
    const FbPixelSplit split = fb_nmf_sweep_split(N, p->num_cu);
    const long long nb = split.workgroups;
    const size_t m = (size_t)N * k + (size_t)k * k + 1;
    // work: [H H^T: 256 | finished sums: m | violations: 2 | partials: nb m]
    const size_t head = 256 + m + 2;
    FB_TRY(p->work.ensure((head + (size_t)nb * m) * sizeof(double)));
    double* hht = p->work.as<double>();
    double* sums = hht + 256;
    double* viol = sums + m;
    double* partial = viol + 2;
    const size_t lds = (size_t)(FB_CLEAN_KMAX * FB_CLEAN_KMAX + 4 * FB_CLEAN_KMAX + 4 * N) * sizeof(double);
    FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_nmf_gram, dim3(1), dim3(256), 0, s, (const double*)H, k, N, hht);
#define FB_NMF_CASE(C_)                                                                                                    \
    hipLaunchKernelGGL((k_nmf_sweep<T, C_>), dim3((unsigned)nb), dim3(256), lds, s, (const T*)cube, W, (const double*)H,   \
                       (const double*)hht, k, npix, N, split.per, partial)
    switch (channels_per_lane(N)) {
        case 1: FB_NMF_CASE(1); break;
        case 2: FB_NMF_CASE(2); break;
        case 4: FB_NMF_CASE(4); break;
        case 8: FB_NMF_CASE(8); break;
        default: FB_NMF_CASE(16); break;
    }
#undef FB_NMF_CASE
    FB_LAUNCH_CHECK("k_nmf_sweep");
    sum_rows(partial, (int)nb, (long long)m, 1.0, sums, s);
    hipLaunchKernelGGL(k_nmf_update_h, dim3(1), dim3(256), 0, s, H, (const double*)sums, k, N, viol);
    FB_LAUNCH_CHECK("k_nmf_update_h");
    FB_TRY(fb_read_back(viol_host, viol, 2 * sizeof(double), s));
    return FB_OK;
}

template <typename T>
int nmf_residual(fb_plan* p, const void* cube, const double* W, const double* H, int k, void* out, double* sumsq_host,
                 hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    long long nb = (npix + 3) / 4;
    if (nb > 2048) nb = 2048;
    FB_TRY(p->work.ensure((size_t)(nb + 1) * sizeof(double)));
    double* partial = p->work.as<double>() + 1;
    { FbProfScope _ps(p, FBK_PCA, s);
#define FB_RES_CASE(C_)                                                                                                    \
    hipLaunchKernelGGL((k_nmf_residual<T, C_>), dim3((unsigned)nb), dim3(256), 0, s, (const T*)cube, W, H, k, npix, N,    \
                       (T*)out, partial)
    switch (channels_per_lane(N)) {
        case 1: FB_RES_CASE(1); break;
        case 2: FB_RES_CASE(2); break;
        case 4: FB_RES_CASE(4); break;
        case 8: FB_RES_CASE(8); break;
        case 16: FB_RES_CASE(16); break;
        case 32: FB_RES_CASE(32); break;
        default: fb_set_error("unsupported grid size"); return FB_ERR_UNSUPPORTED;
    }
#undef FB_RES_CASE
    }
    FB_LAUNCH_CHECK("k_nmf_residual");
    if (sumsq_host) {
        sum_rows(partial, (int)nb, 1, 1.0, p->work.as<double>(), s);
        FB_LAUNCH_CHECK("k_sum_rows");
        FB_TRY(fb_read_back(sumsq_host, p->work, sizeof(double), s));
    }
    return FB_OK;
}

template <typename T>
int rotate_spectra(fb_plan* p, const void* cube, const double* Vt, double* B, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    const unsigned grid = (unsigned)((npix + 3) / 4);
    FbProfScope _ps(p, FBK_PCA, s);
#define FB_ROT_CASE(C_) \
    hipLaunchKernelGGL((k_rotate_spectra<T, C_>), dim3(grid), dim3(256), 0, s, (const T*)cube, Vt, B, npix, N)
    switch (channels_per_lane(N)) {
        case 1: FB_ROT_CASE(1); break;
        case 2: FB_ROT_CASE(2); break;
        case 4: FB_ROT_CASE(4); break;
        case 8: FB_ROT_CASE(8); break;
        case 16: FB_ROT_CASE(16); break;
        case 32: FB_ROT_CASE(32); break;
        default: fb_set_error("unsupported grid size"); return FB_ERR_UNSUPPORTED;
    }
#undef FB_ROT_CASE
    FB_LAUNCH_CHECK("k_rotate_spectra");
    return FB_OK;
}

template <typename T>
int real_min(fb_plan* p, const void* x, double* out_host, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    const int nb = red_blocks(n);
    FB_TRY(p->work.ensure((size_t)(2 * nb + 2) * sizeof(double)));
    double* res = p->work.as<double>();
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_min_finite<T>), dim3(nb), dim3(256), 0, s, (const T*)x, n, res + 2);
    hipLaunchKernelGGL(k_min_finish, dim3(1), dim3(64), 0, s, (const double*)(res + 2), nb, res);
    FB_LAUNCH_CHECK("k_min_finite");
    FB_TRY(fb_read_back(out_host, res, 2 * sizeof(double), s));
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_real_min(fb_plan* p, const void* cube, double* min_out, int64_t* nonfinite_out, void* stream) {
    FB_REQUIRE(p && cube && min_out && nonfinite_out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    double h[2] = {0.0, 0.0};
    const int r = FB_DISPATCH(p, real_min<float>(p, cube, h, s), real_min<double>(p, cube, h, s));
    if (r) return r;
    *min_out = h[0];
    *nonfinite_out = (int64_t)h[1];
    return FB_OK;
}

int fb_complex_to_real(fb_plan* p, const void* full_cube, void* real_cube, void* stream) {
    FB_REQUIRE(p && full_cube && real_cube, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)p->N * p->N * p->N;
    FbProfScope _ps(p, FBK_LAYOUT, s);
    if (p->prec == 4) hipLaunchKernelGGL((k_real_part<float>), dim3(red_blocks(n)), dim3(256), 0, s, (const float*)full_cube, (float*)real_cube, n);
    else hipLaunchKernelGGL((k_real_part<double>), dim3(red_blocks(n)), dim3(256), 0, s, (const double*)full_cube, (double*)real_cube, n);
    FB_LAUNCH_CHECK("k_real_part");
    return FB_OK;
}

// host only, no device: the pixel partitions of k_nmf_sweep on a device of num_cu compute units and of k_ica_step
int fb_nmf_sweep_plan(int N, int num_cu, int* workgroups_out, int64_t* pixels_out) {
    if (N < 2 || N > FB_CLEAN_NMAX || num_cu < 1 || !workgroups_out || !pixels_out) {
        fb_set_error("NMF sweep plan: 2 <= N <= 1024, num_cu >= 1 and two outputs");
        return FB_ERR_INVALID;
    }
    const FbPixelSplit c = fb_nmf_sweep_split(N, num_cu);
    *workgroups_out = c.workgroups;
    *pixels_out = (int64_t)c.per;
    return FB_OK;
}
int fb_ica_step_plan(int N, int* workgroups_out, int64_t* pixels_out) {
    if (N < 2 || !workgroups_out || !pixels_out) {
        fb_set_error("ICA step plan: N >= 2 and two outputs");
        return FB_ERR_INVALID;
    }
    const FbPixelSplit c = fb_ica_step_split(N);
    *workgroups_out = c.workgroups;
    *pixels_out = (int64_t)c.per;
    return FB_OK;
}

int fb_nmf_sweep(fb_plan* p, const void* cube, double* W_dev, double* H_dev, int k, double* violation_out, void* stream) {
    FB_REQUIRE(p && cube && W_dev && H_dev && violation_out, "null pointer");
    FB_REQUIRE(k >= 1 && k <= FB_CLEAN_KMAX, "the number of components must lie in 1 .. 16");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, nmf_sweep<float>(p, cube, W_dev, H_dev, k, violation_out, s),
                       nmf_sweep<double>(p, cube, W_dev, H_dev, k, violation_out, s));
}

int fb_nmf_residual(fb_plan* p, const void* cube, const double* W_dev, const double* H_dev, int k, void* cube_out,
                    double* sumsq_out, void* stream) {
    FB_REQUIRE(p && cube && W_dev && H_dev && (cube_out || sumsq_out), "null pointer");
    FB_REQUIRE(k >= 1 && k <= FB_CLEAN_KMAX, "the number of components must lie in 1 .. 16");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, nmf_residual<float>(p, cube, W_dev, H_dev, k, cube_out, sumsq_out, s),
                       nmf_residual<double>(p, cube, W_dev, H_dev, k, cube_out, sumsq_out, s));
}

int fb_rotated_covariance(fb_plan* p, const void* cube, const double* Vt_dev, double* work_dev, double* cov_dev, void* stream) {
    FB_REQUIRE(p && cube && Vt_dev && work_dev && cov_dev, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)p->N;
    double* zero_mean = work_dev + N * N * N;                      // work: [B: N^2 N | a mean of zeros: N]
    FB_HIP(hipMemsetAsync(zero_mean, 0, N * sizeof(double), s));
    const int r = FB_DISPATCH(p, rotate_spectra<float>(p, cube, Vt_dev, work_dev, s), rotate_spectra<double>(p, cube, Vt_dev, work_dev, s));
    if (r) return r;
    return fbi_channel_cov_f64(p, work_dev, zero_mean, cov_dev, s);     // B is fp64 whatever the plan: the fp64 instance serves both
}

int fb_nndsvd_norms(fb_plan* p, const double* amps_dev, int k, double* out, void* stream) {
    FB_REQUIRE(p && amps_dev && out, "null pointer");
    FB_REQUIRE(k >= 1 && k <= FB_CLEAN_KMAX, "the number of components must lie in 1 .. 16");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)p->N * p->N;
    const int nb = red_blocks(npix);
    FB_TRY(p->work.ensure((size_t)(nb + 1) * 2 * k * sizeof(double)));
    double* res = p->work.as<double>();
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_rows_posneg, dim3(nb), dim3(256), 0, s, amps_dev, k, npix, res + 2 * k);
    sum_rows(res + 2 * k, nb, 2 * k, 1.0, res, s); }
    FB_LAUNCH_CHECK("k_rows_posneg");
    FB_TRY(fb_read_back(out, res, (size_t)2 * k * sizeof(double), s));
    return FB_OK;
}

int fb_nndsvd_fill(fb_plan* p, double* amps_dev, int k, const double* coef, int abs_first, double eps, double fill, void* stream) {
    FB_REQUIRE(p && amps_dev && coef, "null pointer");
    FB_REQUIRE(k >= 1 && k <= FB_CLEAN_KMAX, "the number of components must lie in 1 .. 16");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)p->N * p->N;
    FB_TRY(p->work.ensure(FB_CLEAN_KMAX * sizeof(double)));
    FB_HIP(hipMemcpyAsync(p->work, coef, (size_t)k * sizeof(double), hipMemcpyHostToDevice, s));
    FB_HIP(hipStreamSynchronize(s));                               // `coef` is the caller's
    FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_rows_rectify, dim3(red_blocks(k * npix)), dim3(256), 0, s, amps_dev, k, npix,
                       p->work.as<const double>(), abs_first, eps, fill);
    FB_LAUNCH_CHECK("k_rows_rectify");
    return FB_OK;
}

int fb_ica_step(fb_plan* p, const double* W, const double* X1_dev, int n, int fun, double alpha, double* G_out, double* gp_out,
                void* stream) {
    FB_REQUIRE(p && W && X1_dev && G_out && gp_out, "null pointer");
    FB_REQUIRE(n >= 1 && n <= FB_CLEAN_KMAX, "the number of sources must lie in 1 .. 16");
    FB_REQUIRE(fun == FB_ICA_LOGCOSH || fun == FB_ICA_EXP || fun == FB_ICA_CUBE, "unknown contrast function");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)p->N * p->N;
    const FbPixelSplit split = fb_ica_step_split(p->N);
    const long long nb = split.workgroups;
    const int m = n * n + n;
    // work: [W: 256 | result: m | partials: nb m]
    FB_TRY(p->work.ensure((size_t)(256 + m + nb * m) * sizeof(double)));
    double* wdev = p->work.as<double>();
    double* res = wdev + 256;
    FB_HIP(hipMemcpyAsync(wdev, W, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_ica_step, dim3((unsigned)nb), dim3(256), 0, s, (const double*)wdev, X1_dev, n, npix, split.per, fun,
                       alpha, res + m);
    sum_rows(res + m, (int)nb, m, 1.0 / (double)npix, res, s); }
    FB_LAUNCH_CHECK("k_ica_step");
    double h[FB_CLEAN_KMAX * FB_CLEAN_KMAX + FB_CLEAN_KMAX];
    FB_TRY(fb_read_back(h, res, (size_t)m * sizeof(double), s));
    for (int i = 0; i < n * n; ++i) G_out[i] = h[i];
    for (int i = 0; i < n; ++i) gp_out[i] = h[n * n + i];
    return FB_OK;
}

int fb_ica_sources(fb_plan* p, const double* W, const double* scale, const double* X1_dev, int n, double* sources_dev,
                   double* moments_out, void* stream) {
    FB_REQUIRE(p && W && scale && X1_dev && sources_dev, "null pointer");
    FB_REQUIRE(n >= 1 && n <= FB_CLEAN_KMAX, "the number of sources must lie in 1 .. 16");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)p->N * p->N;
    const int nb = red_blocks(npix);
    // work: [W: 256 | scale: 16 | result: 2 n | partials: nb 2 n]
    FB_TRY(p->work.ensure((size_t)(256 + 16 + 2 * n + (size_t)nb * 2 * n) * sizeof(double)));
    double* wdev = p->work.as<double>();
    double* sdev = wdev + 256;
    double* res = sdev + 16;
    FB_HIP(hipMemcpyAsync(wdev, W, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
    FB_HIP(hipMemcpyAsync(sdev, scale, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_ica_sources, dim3(nb), dim3(256), 0, s, (const double*)wdev, (const double*)sdev, X1_dev, n, npix,
                       sources_dev, res + 2 * n);
    sum_rows(res + 2 * n, nb, 2 * n, 1.0 / (double)npix, res, s); }
    FB_LAUNCH_CHECK("k_ica_sources");
    double h[2 * FB_CLEAN_KMAX];
    FB_TRY(fb_read_back(h, res, (size_t)2 * n * sizeof(double), s));   // also: W and scale are the caller's
    if (moments_out) for (int i = 0; i < 2 * n; ++i) moments_out[i] = h[i];
    return FB_OK;
}

}  // extern "C"
