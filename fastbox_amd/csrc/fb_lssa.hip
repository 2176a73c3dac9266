// Least-squares spectral analysis of flagged cubes (the reference's fastbox/inpaint.py:158-399), for every line of sight of the
// cube at once: each mode's fit is quadratic in its complex amplitude, so the whole cube is four products along the frequency
// axis on the fp64 matrix cores and a small epilogue per (line of sight, mode).  Definitions: DESIGN.md section 4 (LSSA); entry point:
// include/fastbox_hip.h.
//
// The cube is T[pixel = (x, y)][channel], the channel contiguous; a line of sight is one row p of the (N^2, N) view.  With the
// phase tables cos phi[n][j], sin phi[n][j] of the host (mode-major, [Ntau][N]; the device never derives a phase),
// g[p][j] = t_j^2 w^2 / sigma^2 (exactly 0 where w = 0), u = g d (0 where g = 0, whatever d holds there) and v = w^2:
//     A_re[p][n] = sum_j u cos / G_p,  A_im[p][n] = -sum_j u sin / G_p,  G_p = sum_j g
//     S_cc = sum_j v cos^2,  S_cs = sum_j v cos sin,  S_ss = W_p - S_cc,  W_p = sum_j v
// and the decorrelated power of lssa_power below.  Every sum is formed in a fixed order: no floating-point atomics, results
// are bitwise repeatable.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <cmath>

#define FB_LSSA_NMAX 1024                // channels, and modes
#define FB_LSSA_MP 2                     // 16-pixel tiles of a wave
#define FB_LSSA_MT 2                     // 16-mode tiles of a wave

namespace {
using namespace fb;

typedef double fb_d4 __attribute__((ext_vector_type(4)));
typedef double fb_d2 __attribute__((ext_vector_type(2)));
typedef float fb_f4 __attribute__((ext_vector_type(4)));

// four consecutive elements as they are stored (converted where they are used, so that a fetch does not wait for its data)
__device__ __forceinline__ void raw4(const double* __restrict__ src, double (&v)[4]) {
    const fb_d2 a = *reinterpret_cast<const fb_d2*>(src), b = *reinterpret_cast<const fb_d2*>(src + 2);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
}
__device__ __forceinline__ void raw4(const float* __restrict__ src, float (&v)[4]) {
    const fb_f4 a = *reinterpret_cast<const fb_f4*>(src);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}

struct LssaArgs {
    const void* d;           // cube in the plan's precision (FIT)
    const void* w;           // cube in the plan's precision (PV)
    const void* var;         // cube in the plan's precision (VV)
    const double* gc;        // [N] the per-channel part of g: t^2, times w^2 and over sigma^2 where those are per channel
    const double* tc;        // [ntau][N] cos phi
    const double* ts;        // [ntau][N] sin phi
    const double* S;         // [3][ntau] S_cc, S_cs, S_ss of per-channel flags (!PV)
    const double* G;         // [npix]
    const double* W;         // [npix] (PV)
    double* A_re;            // [npix][ntau] or NULL; read, not written, without FIT
    double* A_im;
    double* ps;              // [npix][ntau] or NULL
    double* partial;         // [2][ntau][nblk]: sum of ps and of ps^2 over the 32 pixels of a wave
    long long npix;
    long long nblk;
    int N, ntau, decorr;
};

// the rotation that decorrelates the cosine and sine amplitudes of a mode, and the eigenvalues of their overlap matrix
// (lssa_decorr_matrix, inpaint.py:343-359, formula for formula)
__device__ __forceinline__ void lssa_rotation(double scc, double scs, double sss, double& cs, double& sn, double& l0, double& l1) {
#pragma clang fp contract(off)
    const double th = 0.5 * atan2(2.0 * scs, scc - sss);
    sincos(th, &sn, &cs);
    l0 = cs * cs * scc + 2.0 * sn * cs * scs + sn * sn * sss;
    l1 = sn * sn * scc - 2.0 * sn * cs * scs + cs * cs * sss;
}
// lssa_pspec (inpaint.py:393-398); without the decorrelation |A|^2
__device__ __forceinline__ double lssa_power(double are, double aim, double cs, double sn, double l0, double l1, int decorr) {
#pragma clang fp contract(off)
    if (!decorr) return are * are + aim * aim;
    const double x = (cs * are + sn * aim) * l1, y = (-sn * are + cs * aim) * l0;
    return (x * x + y * y) / (l0 * l0 + l1 * l1);
}

// The fused kernel on v_mfma_f64_16x16x4_f64, operand layout and chunk order as documented at k_los_matmul (fb_inpaint.hip) and
// k_channel_cov (fb_field_kernels.h): the A operand is 16 pixels x 4 channels (lane l: pixel l & 15, k = l >> 4), formed on the
// fly -- u = g d for the two amplitude sums and, with per-voxel flags (PV), v = w^2 for the two overlap sums; the B operand is 4
// channels x 16 modes (lane l: k = l >> 4, mode l & 15), read from row n of the mode-major tables cos phi and sin phi (cos^2
// phi and cos phi sin phi are products of the two values in registers: half the table traffic and registers); D has the mode
// l & 15 on the lane and pixel (l >> 4) + 4 reg in the registers, so a wave's stores are 128-byte runs along the mode axis.
// Lane group k = l >> 4 of the j-th instruction of a 16-channel chunk takes channel b0 + 4 k + j.
// One wave owns 32 pixels x 32 modes and up to four accumulator sets of 2 x 2 tiles (sum u cos, sum u sin, sum v cos^2, sum v
// cos sin: 128 accumulator registers) over the whole sum, at one wave per SIMD (two with per-channel flags); the four waves of a workgroup cover 64 pixels x
// 64 modes and share their rows through L1.  Operands are fetched one chunk ahead of the matrix instructions that use them, as
// stored; the conversion and the weights are applied after the wait.
// VV: sigma^2 is a cube.  FIT: the amplitudes are fitted (else A_re, A_im are read and only the power is formed; with
// per-channel flags that leaves no product at all).  EDGE: N is not a multiple of 16, or N^2 or Ntau of 32: rows, channels
// and modes past the end read a valid address, count as 0 and are not stored.
// Epilogue, in registers: divide by G_p, rotate, form ps, store what is asked for, and sum ps and ps^2 over the wave's pixels
// with G_p > 0 (pixels ascending on the lane, then the four lane groups by two exchanges) into partial[.][n][wave's pixel block].
template <typename T, bool PV, bool VV, bool FIT, bool EDGE>
__global__ __launch_bounds__(256) void k_lssa(const LssaArgs a) {
    constexpr int MP = FB_LSSA_MP, MT = FB_LSSA_MT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
    const int N = a.N, ntau = a.ntau;
    const long long npix = a.npix;
    const long long pblk = (long long)blockIdx.x * 2 + (wave & 1);
    const long long p0 = pblk * (16 * MP);
    const int n0 = blockIdx.y * (32 * MT) + 16 * MT * (wave >> 1);
    if (n0 >= ntau || p0 >= npix) return;               // wave-uniform; the kernel has no barrier
    const T* __restrict__ dd = (const T*)a.d;
    const T* __restrict__ ww = (const T*)a.w;
    const T* __restrict__ vv = (const T*)a.var;
    long long xrow[MP];
    bool xok[MP], tok[MT];
    size_t trow[MT];
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        xrow[i] = p0 + 16 * i + lc; xok[i] = !EDGE || xrow[i] < npix;
        if (EDGE && !xok[i]) xrow[i] = npix - 1;
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        int n = n0 + 16 * j + lc;
        tok[j] = !EDGE || n < ntau;
        if (EDGE && !tok[j]) n = ntau - 1;
        trow[j] = (size_t)n * N;
    }
    // accumulator sets: 0 sum u cos, 1 sum u sin, 2 sum v cos^2, 3 sum v cos sin
    fb_d4 acc[4][MP][MT];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < MP; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) acc[q][i][j] = fb_d4{0.0, 0.0, 0.0, 0.0};

    if constexpr (FIT || PV) {
        T dr[2][MP][4], wr[2][MP][4], vr[2][MP][4];
        double gr[2][4], tb[2][MT][2][4];
        auto fetch = [&](int buf, int b0) {
            const int b = b0 + 4 * lk;
            if constexpr (!EDGE) {
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    if constexpr (FIT) raw4(dd + xrow[i] * N + b, dr[buf][i]);
                    if constexpr (PV) raw4(ww + xrow[i] * N + b, wr[buf][i]);
                    if constexpr (FIT && VV) raw4(vv + xrow[i] * N + b, vr[buf][i]);
                }
                if constexpr (FIT) raw4(a.gc + b, gr[buf]);
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    raw4(a.tc + trow[j] + b, tb[buf][j][0]);
                    raw4(a.ts + trow[j] + b, tb[buf][j][1]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool cok = b + u < N;
                    const int c = cok ? b + u : N - 1;
#pragma unroll
                    for (int i = 0; i < MP; ++i) {
                        if constexpr (FIT) dr[buf][i][u] = dd[xrow[i] * N + c];
                        if constexpr (PV) { const T v = ww[xrow[i] * N + c]; wr[buf][i][u] = (cok && xok[i]) ? v : (T)0; }
                        if constexpr (FIT && VV) vr[buf][i][u] = vv[xrow[i] * N + c];
                    }
                    if constexpr (FIT) { const double v = a.gc[c]; gr[buf][u] = cok ? v : 0.0; }   // (a row past the end is not stored)
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
                        const bool ok = cok && tok[j];
                        const double c1 = a.tc[trow[j] + c], s1 = a.ts[trow[j] + c];
                        tb[buf][j][0][u] = ok ? c1 : 0.0; tb[buf][j][1][u] = ok ? s1 : 0.0;
                    }
                }
            }
        };
        auto update = [&](int buf) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                double c2[MT], cs[MT];                  // cos^2 phi, cos phi sin phi: products of table values, each rounded once
#pragma unroll
                for (int j = 0; j < MT; ++j) { c2[j] = tb[buf][j][0][u] * tb[buf][j][0][u]; cs[j] = tb[buf][j][0][u] * tb[buf][j][1][u]; }
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    double uval = 0.0, vval = 0.0;
                    if constexpr (PV) {
                        const double wv = (double)wr[buf][i][u];
                        vval = wv * wv;
                        if constexpr (FIT) {
                            double g = gr[buf][u] * vval;
                            if constexpr (VV) g = g / (double)vr[buf][i][u];
                            g = wv != 0.0 ? g : 0.0;
                            uval = g != 0.0 ? g * (double)dr[buf][i][u] : 0.0;
                        }
                    } else {
                        double g = gr[buf][u];
                        if constexpr (VV) g = g != 0.0 ? g / (double)vr[buf][i][u] : 0.0;
                        uval = g != 0.0 ? g * (double)dr[buf][i][u] : 0.0;
                    }
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
                        if constexpr (FIT) {
                            acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(uval, tb[buf][j][0][u], acc[0][i][j], 0, 0, 0);
                            acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(uval, tb[buf][j][1][u], acc[1][i][j], 0, 0, 0);
                        }
                        if constexpr (PV) {
                            acc[2][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(vval, c2[j], acc[2][i][j], 0, 0, 0);
                            acc[3][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(vval, cs[j], acc[3][i][j], 0, 0, 0);
                        }
                    }
                }
            }
        };
        fetch(0, 0);
        for (int b0 = 0; b0 < N; b0 += 32) {
            if (b0 + 16 < N) fetch(1, b0 + 16);
            update(0);
            if (b0 + 16 < N) {
                if (b0 + 32 < N) fetch(0, b0 + 32);
                update(1);
            }
        }
    }

    // ---- epilogue ----
    double cs[MT], sn[MT], l0[MT], l1[MT], s1[MT], s2[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        s1[j] = s2[j] = 0.0;
        cs[j] = 1.0; sn[j] = l0[j] = l1[j] = 0.0;
        if constexpr (!PV) {
            const int n = n0 + 16 * j + lc;
            if (a.decorr && (!EDGE || n < ntau)) lssa_rotation(a.S[n], a.S[ntau + n], a.S[2 * ntau + n], cs[j], sn[j], l0[j], l1[j]);
        }
    }
#pragma unroll
    for (int i = 0; i < MP; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = p0 + 16 * i + lk + 4 * r;
            const bool pok = !EDGE || p < npix;
            const double G = a.G[pok ? p : npix - 1];
            const bool on = pok && G > 0.0;
            double Wp = 0.0;
            if constexpr (PV) Wp = a.W[pok ? p : npix - 1];
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int n = n0 + 16 * j + lc;
                const bool ok = pok && (!EDGE || n < ntau);
                const long long o = ok ? p * ntau + n : 0;
                double are = 0.0, aim = 0.0;
                if constexpr (FIT) {
                    if (on) { are = acc[0][i][j][r] / G; aim = -acc[1][i][j][r] / G; }
                } else if (on && ok) { are = a.A_re[o]; aim = a.A_im[o]; }
                double c = cs[j], s = sn[j], e0 = l0[j], e1 = l1[j];
                if constexpr (PV) {
                    const double scc = acc[2][i][j][r];
                    if (a.decorr) lssa_rotation(scc, acc[3][i][j][r], Wp - scc, c, s, e0, e1);
                }
                const double ps = on ? lssa_power(are, aim, c, s, e0, e1, a.decorr) : NAN;
                if (ok) {
                    if constexpr (FIT) {
                        if (a.A_re) a.A_re[o] = are;
                        if (a.A_im) a.A_im[o] = aim;
                    }
                    if (a.ps) a.ps[o] = ps;
                    if (on) { s1[j] += ps; s2[j] += ps * ps; }
                }
            }
        }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        double x = s1[j], y = s2[j];
        x += __shfl_xor(x, 16, 64); y += __shfl_xor(y, 16, 64);
        x += __shfl_xor(x, 32, 64); y += __shfl_xor(y, 32, 64);
        const int n = n0 + 16 * j + lc;
        if (lk == 0 && (!EDGE || n < ntau)) {
            a.partial[(size_t)n * a.nblk + pblk] = x;
            a.partial[((size_t)ntau + n) * a.nblk + pblk] = y;
        }
    }
}

// gc[j] = t_j^2, times w_j^2 and over sigma_j^2 where those come per channel; exactly 0 where w_j = 0
__global__ __launch_bounds__(256) void k_lssa_channels(const double* __restrict__ w, const double* __restrict__ var,
                                                       const double* __restrict__ taper, double* __restrict__ gc, int N) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const double t = taper ? taper[c] : 1.0;
    double g = t * t;
    if (w) { const double wv = w[c]; g = wv != 0.0 ? g * (wv * wv) : 0.0; }
    if (var && g != 0.0) g = g / var[c];
    gc[c] = g;
}

// G_p = sum_j g, W_p = sum_j w^2: one wave per line of sight, lane l holds channels l, l + 64, ... in ascending order, then a
// butterfly over the wave
template <typename T, bool PV, bool VV>
__global__ __launch_bounds__(256) void k_lssa_rowsums(const T* __restrict__ w, const T* __restrict__ var, const double* __restrict__ gc,
                                                      double* __restrict__ G, double* __restrict__ W, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;
    double sg = 0.0, sw = 0.0;
    for (int c = lane; c < N; c += 64) {
        double g = gc[c];
        if constexpr (PV) {
            const double wv = (double)w[p * N + c], v = wv * wv;
            g = g * v;
            if constexpr (VV) g = g / (double)var[p * N + c];
            g = wv != 0.0 ? g : 0.0;
            sw += v;
        } else if constexpr (VV) {
            g = g != 0.0 ? g / (double)var[p * N + c] : 0.0;
        }
        sg += g;
    }
    sg = wave_sum(sg);
    if constexpr (PV) sw = wave_sum(sw);
    if (lane == 0) {
        G[p] = sg;
        if constexpr (PV) W[p] = sw;
    }
}

// out = [mean of ps: ntau | population standard deviation / sqrt(n_los): ntau | n_los] from sums = [sum ps: ntau | sum ps^2:
// ntau] over the n_los lines of sight with G_p > 0; one workgroup, the count in integers
__global__ __launch_bounds__(1024) void k_lssa_stats(const double* __restrict__ G, long long npix, const double* __restrict__ sums,
                                                     int ntau, double* __restrict__ out) {
    __shared__ long long cnt[1024];
    long long c = 0;
    for (long long p = threadIdx.x; p < npix; p += 1024) c += G[p] > 0.0 ? 1 : 0;
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
        __syncthreads();
    }
    const double n = (double)cnt[0];
    for (int q = threadIdx.x; q < ntau; q += 1024) {
        const double mean = sums[q] / n, var = sums[ntau + q] / n - mean * mean;
        out[q] = mean;
        out[ntau + q] = sqrt(var > 0.0 ? var : (var == var ? 0.0 : var)) / sqrt(n);
    }
    if (threadIdx.x == 0) out[2 * ntau] = n;
}

template <typename T, bool PV, bool VV, bool FIT>
void launch_lssa(const LssaArgs& a, bool edge, dim3 grid, hipStream_t s) {
    if (edge) hipLaunchKernelGGL((k_lssa<T, PV, VV, FIT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_lssa<T, PV, VV, FIT, false>), grid, dim3(256), 0, s, a);
}

template <typename T>
int lssa(fb_plan* p, LssaArgs a, const double* w_chan, const double* var_chan, const double* taper, bool pv, bool vv, bool fit,
         double* mean_out, double* stderr_out, long long* n_los_out, hipStream_t s) {
    const int N = p->N, ntau = a.ntau;
    const long long npix = (long long)N * N;
    const long long nblk = (npix + 16 * FB_LSSA_MP - 1) / (16 * FB_LSSA_MP);
    // work: [gc: N | G: npix | W: npix | sums: 2 ntau | out: 2 ntau + 1 | partial: 2 ntau nblk]
    const size_t head = (size_t)N + 2 * (size_t)npix + 4 * (size_t)ntau + 1;
    FB_TRY(p->work.ensure((head + 2 * (size_t)ntau * (size_t)nblk) * sizeof(double)));
    double* gc = p->work.as<double>();
    double* G = gc + N;
    double* W = G + npix;
    double* sums = W + npix;
    double* out = sums + 2 * ntau;
    double* partial = out + 2 * ntau + 1;
    a.gc = gc; a.G = G; a.W = W; a.partial = partial; a.npix = npix; a.nblk = nblk; a.N = N;
    FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_lssa_channels, dim3((N + 255) / 256), dim3(256), 0, s, w_chan, var_chan, taper, gc, N);
    const dim3 rows((unsigned)((npix + 3) / 4));
    const T* wc = (const T*)a.w;
    const T* vc = (const T*)a.var;
    if (pv && vv) hipLaunchKernelGGL((k_lssa_rowsums<T, true, true>), rows, dim3(256), 0, s, wc, vc, (const double*)gc, G, W, npix, N);
    else if (pv) hipLaunchKernelGGL((k_lssa_rowsums<T, true, false>), rows, dim3(256), 0, s, wc, vc, (const double*)gc, G, W, npix, N);
    else if (vv) hipLaunchKernelGGL((k_lssa_rowsums<T, false, true>), rows, dim3(256), 0, s, wc, vc, (const double*)gc, G, W, npix, N);
    else hipLaunchKernelGGL((k_lssa_rowsums<T, false, false>), rows, dim3(256), 0, s, wc, vc, (const double*)gc, G, W, npix, N);
    FB_LAUNCH_CHECK("k_lssa_rowsums");
    const dim3 grid((unsigned)((nblk + 1) / 2), (unsigned)((ntau + 32 * FB_LSSA_MT - 1) / (32 * FB_LSSA_MT)));
    const bool edge = N % 16 != 0 || npix % (16 * FB_LSSA_MP) != 0 || ntau % (16 * FB_LSSA_MT) != 0;
    if (fit) {
        if (pv && vv) launch_lssa<T, true, true, true>(a, edge, grid, s);
        else if (pv) launch_lssa<T, true, false, true>(a, edge, grid, s);
        else if (vv) launch_lssa<T, false, true, true>(a, edge, grid, s);
        else launch_lssa<T, false, false, true>(a, edge, grid, s);
    } else {                                            // the power alone does not read sigma^2 beyond G
        if (pv) launch_lssa<T, true, false, false>(a, edge, grid, s);
        else launch_lssa<T, false, false, false>(a, edge, grid, s);
    }
    FB_LAUNCH_CHECK("k_lssa");
    hipLaunchKernelGGL(k_bin_finish<>, dim3(2 * ntau), dim3(256), 0, s, (const double*)partial, (int)nblk, 2 * ntau, sums);
    hipLaunchKernelGGL(k_lssa_stats, dim3(1), dim3(1024), 0, s, (const double*)G, npix, (const double*)sums, ntau, out);
    FB_LAUNCH_CHECK("k_lssa_stats");
    double h[2 * FB_LSSA_NMAX + 1];
    FB_TRY(fb_read_back(h, out, (size_t)(2 * ntau + 1) * sizeof(double), s));
    for (int n = 0; n < ntau; ++n) {
        if (mean_out) mean_out[n] = h[n];
        if (stderr_out) stderr_out[n] = h[ntau + n];
    }
    if (n_los_out) *n_los_out = (long long)h[2 * ntau];
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_lssa(fb_plan* p, const void* d, const void* w, int w_kind, const void* var, int var_kind, const double* taper_dev,
            const double* cos_dev, const double* sin_dev, const double* s_dev, int ntau, int decorrelate, int amps_given, double* A_re, double* A_im, double* ps, double* ps_mean_out,
            double* ps_stderr_out, long long* n_los_out, void* stream) {
    FB_REQUIRE(p && w, "null pointer");
    FB_REQUIRE((w_kind == FB_GCR_PER_CHANNEL || w_kind == FB_GCR_PER_VOXEL) && (var_kind == FB_GCR_PER_CHANNEL || var_kind == FB_GCR_PER_VOXEL),
               "w_kind, var_kind: FB_GCR_PER_CHANNEL or FB_GCR_PER_VOXEL");
    FB_REQUIRE(p->N <= FB_LSSA_NMAX && ntau >= 1 && ntau <= FB_LSSA_NMAX, "fb_lssa: at most 1024 channels and 1 .. 1024 modes");
    FB_REQUIRE(amps_given ? (A_re && A_im) : d != nullptr, "fb_lssa: d, or amps_given with A_re and A_im");
    const bool pv = w_kind == FB_GCR_PER_VOXEL, vv = var && var_kind == FB_GCR_PER_VOXEL;
    FB_REQUIRE((cos_dev && sin_dev) || (amps_given && !pv), "fb_lssa: the cos and sin tables");
    FB_REQUIRE(pv || !decorrelate || s_dev, "fb_lssa: per-channel flags need s_dev for the decorrelation");
    FB_REQUIRE(!ps || (ps != A_re && ps != A_im), "fb_lssa: ps must not be A_re or A_im");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    LssaArgs a = {};
    a.d = d; a.w = pv ? w : nullptr; a.var = vv ? var : nullptr;
    a.tc = cos_dev; a.ts = sin_dev;
    a.S = s_dev; a.A_re = A_re; a.A_im = A_im; a.ps = ps; a.ntau = ntau; a.decorr = decorrelate ? 1 : 0;
    const double* w_chan = pv ? nullptr : (const double*)w;
    const double* var_chan = (var && !vv) ? (const double*)var : nullptr;
    const bool fit = !amps_given;
    return FB_DISPATCH(p, lssa<float>(p, a, w_chan, var_chan, taper_dev, pv, vv, fit, ps_mean_out, ps_stderr_out, n_los_out, s),
                       lssa<double>(p, a, w_chan, var_chan, taper_dev, pv, vv, fit, ps_mean_out, ps_stderr_out, n_los_out, s));
}

}  // extern "C"
