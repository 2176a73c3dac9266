// In-painting of flagged channels by Gaussian constrained realisations (the reference's fastbox/inpaint.py:35-155), for every
// line of sight of the cube at once: the product along the frequency axis on the fp64 matrix cores, the batched preconditioned
// conjugate-gradient loop, and the elementwise kernels before and after it.  Definitions: DESIGN.md section 4; entry points:
// include/fastbox_hip.h.
//
// The cube is T[pixel = (x, y)][channel], the channel contiguous; a line of sight is one row of the (N^2, N) view.  All solver
// state is fp64 whatever the plan's precision.  Every sum is formed in a fixed order (lane partials, then a butterfly over
// the wave): no floating-point atomics, results are bitwise repeatable.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include "fb_rng.h"
#include <cmath>

#define FB_GCR_NMAX 1024                 // channels: nine fp64 cubes of working memory are 72 GiB there
#define FB_GCR_STREAM_OMEGA1 7u          // Philox streams of the three unit-normal cubes (0 .. 6 are taken)
#define FB_GCR_STREAM_OMEGA2 8u
#define FB_GCR_STREAM_OMEGA3 9u

namespace {
using namespace fb;

typedef double fb_d4 __attribute__((ext_vector_type(4)));
typedef double fb_d2 __attribute__((ext_vector_type(2)));
typedef float fb_f4 __attribute__((ext_vector_type(4)));

// four consecutive elements, 16-byte aligned where T is float and 32-byte aligned (read as two halves) where it is double
__device__ __forceinline__ void load4(const double* __restrict__ src, double (&v)[4]) {
    const fb_d2 a = *reinterpret_cast<const fb_d2*>(src), b = *reinterpret_cast<const fb_d2*>(src + 2);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
}
__device__ __forceinline__ void load4(const float* __restrict__ src, double (&v)[4]) {
    const fb_f4 a = *reinterpret_cast<const fb_f4*>(src);
    v[0] = (double)a[0]; v[1] = (double)a[1]; v[2] = (double)a[2]; v[3] = (double)a[3];
}

// Y[p][a] = post[p][a] sum_b M[a][b] (pre[p][b] X[p][b]) + add[p][a] on v_mfma_f64_16x16x4_f64, operand layout as documented
// at k_channel_cov (fb_field_kernels.h): A is 16 pixels x 4 channels b (lane l: pixel l & 15, k = l >> 4), B is 4 channels b x 16
// channels a (lane l: k = l >> 4, a = l & 15, read from row a of M -- M is not transposed and not assumed symmetric), D has
// a = l & 15 on the lane and pixel (l >> 4) + 4 reg in the registers, so a wave's stores are 128-byte runs along the channel
// axis.  The sum over b may be taken in any order as long as both operands agree on it: lane group k = l >> 4 of the j-th
// instruction of a 16-channel chunk takes channel b0 + 4 k + j, so that every lane reads 32 contiguous bytes of its row of X
// and of its row of M per chunk and a chunk consumes whole 128-byte lines of both.
// One wave owns 32 pixels x 64 channels (2 x 4 accumulators of 8 VGPRs) over the whole sum; the four waves of a workgroup
// cover 64 pixels x 128 channels and share their rows of X and M through L1.  Operands come straight from global memory (M is
// N^2 doubles and stays in L2), fetched one chunk ahead of the matrix instructions that use them.
// EDGE: N is not a multiple of 64 (or N^2 of 64): rows and channels past the end read a valid address, count as 0 and are
// not stored.
#define FB_LOS_MP 2
#define FB_LOS_MC 4
template <typename TX, bool EDGE>
__global__ __launch_bounds__(256) void k_los_matmul(const double* __restrict__ M, const TX* __restrict__ X,
                                                    const double* __restrict__ pre, const double* __restrict__ post,
                                                    const double* add, double* Y, long long npix, int N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
    const long long p0 = (long long)blockIdx.x * (32 * FB_LOS_MP) + 16 * FB_LOS_MP * (wave & 1);
    const int a0 = blockIdx.y * (32 * FB_LOS_MC) + 16 * FB_LOS_MC * (wave >> 1);
    if (a0 >= N || p0 >= npix) return;                  // wave-uniform; the kernel has no barrier
    long long xrow[FB_LOS_MP];
    bool xok[FB_LOS_MP], mok[FB_LOS_MC];
    int mrow[FB_LOS_MC];
#pragma unroll
    for (int i = 0; i < FB_LOS_MP; ++i) {
        xrow[i] = p0 + 16 * i + lc; xok[i] = !EDGE || xrow[i] < npix;
        if (EDGE && !xok[i]) xrow[i] = npix - 1;
    }
#pragma unroll
    for (int j = 0; j < FB_LOS_MC; ++j) {
        mrow[j] = a0 + 16 * j + lc; mok[j] = !EDGE || mrow[j] < N;
        if (EDGE && !mok[j]) mrow[j] = N - 1;
    }
    fb_d4 acc[FB_LOS_MP][FB_LOS_MC];
#pragma unroll
    for (int i = 0; i < FB_LOS_MP; ++i)
#pragma unroll
        for (int j = 0; j < FB_LOS_MC; ++j) acc[i][j] = fb_d4{0.0, 0.0, 0.0, 0.0};
    double xv[2][FB_LOS_MP][4], mv[2][FB_LOS_MC][4];
    auto fetch = [&](int buf, int b0) {
        const int b = b0 + 4 * lk;
        if (!EDGE) {
#pragma unroll
            for (int i = 0; i < FB_LOS_MP; ++i) {
                load4(X + xrow[i] * N + b, xv[buf][i]);
                if (pre) {
                    double pv[4];
                    load4(pre + xrow[i] * N + b, pv);
#pragma unroll
                    for (int u = 0; u < 4; ++u) xv[buf][i][u] *= pv[u];
                }
            }
#pragma unroll
            for (int j = 0; j < FB_LOS_MC; ++j) load4(M + (size_t)mrow[j] * N + b, mv[buf][j]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool cok = b + u < N;
                const int c = cok ? b + u : N - 1;
#pragma unroll
                for (int i = 0; i < FB_LOS_MP; ++i) {
                    double v = (double)X[xrow[i] * N + c];
                    if (pre) v *= pre[xrow[i] * N + c];
                    xv[buf][i][u] = (cok && xok[i]) ? v : 0.0;
                }
#pragma unroll
                for (int j = 0; j < FB_LOS_MC; ++j) {
                    const double v = M[(size_t)mrow[j] * N + c];
                    mv[buf][j][u] = (cok && mok[j]) ? v : 0.0;
                }
            }
        }
    };
    auto update = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < FB_LOS_MP; ++i)
#pragma unroll
                for (int j = 0; j < FB_LOS_MC; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[buf][i][u], mv[buf][j][u], acc[i][j], 0, 0, 0);
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
#pragma unroll
    for (int i = 0; i < FB_LOS_MP; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = p0 + 16 * i + lk + 4 * r;
#pragma unroll
            for (int j = 0; j < FB_LOS_MC; ++j) {
                const int a = a0 + 16 * j + lc;
                if (!EDGE || (p < npix && a < N)) {
                    const long long o = p * N + a;
                    double v = acc[i][j][r];
                    if (post) v *= post[o];
                    if (add) v += add[o];
                    Y[o] = v;
                }
            }
        }
}

// ---- the right-hand side -------------------------------------------------------------------------------------------------------
// weight and variance of voxel (p, c): flags per voxel (T) or per channel (fp64), variance per channel (fp64) or per voxel (T)
template <typename T>
__device__ __forceinline__ double flag_at(const void* w, int w_kind, long long i, int c) {
    return w_kind == FB_GCR_PER_CHANNEL ? ((const double*)w)[c] : (double)((const T*)w)[i];
}
template <typename T>
__device__ __forceinline__ double var_at(const void* var, int var_kind, long long i, int c) {
    return var_kind == FB_GCR_PER_CHANNEL ? ((const double*)var)[c] : (double)((const T*)var)[i];
}

// q = w^2 / sigma^2 (exactly 0 where w = 0), u = q d + sqrt(q) omega2 (d is not read arithmetically where w = 0: a NaN under
// a flag is legal), and the omega1 cube when it comes from the generator.  draws: FB_GCR_DRAWS_*.
template <typename T>
__global__ __launch_bounds__(256) void k_gcr_rhs(const T* __restrict__ d, const void* __restrict__ w, int w_kind,
                                                 const void* __restrict__ var, int var_kind, const double* __restrict__ omega2,
                                                 int draws, fb::RngKey key, double* __restrict__ q_out, double* __restrict__ u_out,
                                                 double* __restrict__ omega1_out, long long n, int N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % N);
        const double wv = flag_at<T>(w, w_kind, i, c);
        double q = 0.0, u = 0.0;
        if (wv != 0.0) {
            q = wv * wv / var_at<T>(var, var_kind, i, c);
            u = q * (double)d[i];
            if (draws == FB_GCR_DRAWS_GIVEN) u += sqrt(q) * omega2[i];
            else if (draws == FB_GCR_DRAWS_DEVICE) u += sqrt(q) * fb::stream_noise_at<double>((unsigned long long)i, FB_GCR_STREAM_OMEGA2, key);
        }
        q_out[i] = q;
        u_out[i] = u;
        if (draws == FB_GCR_DRAWS_DEVICE) omega1_out[i] = fb::stream_noise_at<double>((unsigned long long)i, FB_GCR_STREAM_OMEGA1, key);
    }
}

// out = s (+ sigma omega3), or with `inpaint` d where w != 0 and that elsewhere; stored in the plan's precision
template <typename T>
__global__ __launch_bounds__(256) void k_gcr_finish(const double* __restrict__ s, const void* __restrict__ var, int var_kind,
                                                    const double* __restrict__ omega3, int noise, fb::RngKey key,
                                                    const T* __restrict__ d, const void* __restrict__ w, int w_kind, int inpaint,
                                                    T* __restrict__ out, long long n, int N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % N);
        if (inpaint && flag_at<T>(w, w_kind, i, c) != 0.0) { out[i] = d[i]; continue; }
        double v = s[i];
        if (noise == FB_GCR_DRAWS_GIVEN) v += sqrt(var_at<T>(var, var_kind, i, c)) * omega3[i];
        else if (noise == FB_GCR_DRAWS_DEVICE)
            v += sqrt(var_at<T>(var, var_kind, i, c)) * fb::stream_noise_at<double>((unsigned long long)i, FB_GCR_STREAM_OMEGA3, key);
        out[i] = (T)v;
    }
}

// ---- per-row kernels of the conjugate-gradient loop: one wave per line of sight, lane l holds channels l, l + 64, ... ----------
struct GcrRows {
    double* rz;          // [npix] r . z of the current direction
    double* bb;          // [npix] |b|^2
    int* active;         // [npix] 1 while the row iterates
    int32_t* n_iter;     // [npix]
    int* count;          // active rows after the step
};

// x = 0, r = b, |b|^2; a row with b = 0 never starts
__global__ __launch_bounds__(256) void k_cg_init(const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r,
                                                 GcrRows st, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;
    double s = 0.0;
    for (int c = lane; c < N; c += 64) {
        const double v = b[p * N + c];
        x[p * N + c] = 0.0; r[p * N + c] = v;
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const int on = s > 0.0 ? 1 : 0;             // (a NaN in b leaves the row off; the final residual reports it)
        st.bb[p] = s; st.rz[p] = 0.0; st.active[p] = on; st.n_iter[p] = 0;
        if (on) atomicAdd(st.count, 1);
    }
}

// alpha = r.z / p.Ap; x += alpha p; r -= alpha Ap; the row stops once |r| <= tol |b|.  A stopped row is not touched.
__global__ __launch_bounds__(256) void k_cg_step(const double* __restrict__ pd, const double* __restrict__ ap, double* __restrict__ x,
                                                 double* __restrict__ r, GcrRows st, double tol2, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix || !st.active[p]) return;
    double s = 0.0;
    for (int c = lane; c < N; c += 64) s += pd[p * N + c] * ap[p * N + c];
    s = wave_sum(s);
    const double rz = st.rz[p];
    const double alpha = (s != 0.0 && s == s) ? rz / s : 0.0;          // 0 / 0 selects 0
    double rr = 0.0;
    for (int c = lane; c < N; c += 64) {
        const long long i = p * N + c;
        x[i] += alpha * pd[i];
        const double v = r[i] - alpha * ap[i];
        r[i] = v;
        rr += v * v;
    }
    rr = wave_sum(rr);
    if (lane == 0) {
        st.n_iter[p] += 1;
        if (rr <= tol2 * st.bb[p] || alpha == 0.0) st.active[p] = 0;   // alpha = 0: no progress is possible any more
        else atomicAdd(st.count, 1);
    }
}

// beta = (r.z)_new / (r.z)_old (0 on the first call and where the old value is 0), p = z + beta p
__global__ __launch_bounds__(256) void k_cg_direction(const double* __restrict__ r, const double* __restrict__ z, double* __restrict__ pd,
                                                      GcrRows st, int first, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix || !st.active[p]) return;
    double s = 0.0;
    for (int c = lane; c < N; c += 64) s += r[p * N + c] * z[p * N + c];
    s = wave_sum(s);
    const double old = st.rz[p];
    const double beta = (first || old == 0.0) ? 0.0 : s / old;
    for (int c = lane; c < N; c += 64) {
        const long long i = p * N + c;
        pd[i] = first ? z[i] : z[i] + beta * pd[i];
    }
    if (lane == 0) st.rz[p] = s;
}

// res[p] = |b - A x| / |b| (0 where b = 0)
__global__ __launch_bounds__(256) void k_row_residual(const double* __restrict__ b, const double* __restrict__ ax, GcrRows st,
                                                      double* __restrict__ res, long long npix, int N) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;
    double s = 0.0;
    for (int c = lane; c < N; c += 64) { const double v = b[p * N + c] - ax[p * N + c]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) {
        const double bb = st.bb[p];
        res[p] = bb > 0.0 ? sqrt(s / bb) : (bb == 0.0 ? 0.0 : NAN);
    }
}
// out[0] = max res (NaN if any is), out[1] = rows that have stopped (met the tolerance, or b = 0), out[2] = max n_iter: one
// workgroup, fixed order
__global__ __launch_bounds__(1024) void k_gcr_summary(const double* __restrict__ res, const int32_t* __restrict__ n_iter,
                                                      const int* __restrict__ active, long long npix, double* __restrict__ out) {
    __shared__ double sm[1024], sc[1024], si[1024];
    double m = 0.0, cnt = 0.0, it = 0.0;
    bool bad = false;
    for (long long p = threadIdx.x; p < npix; p += 1024) {
        const double v = res[p];
        if (v != v) bad = true; else m = fmax(m, v);
        if (!active[p] && v == v) cnt += 1.0;
        it = fmax(it, (double)n_iter[p]);
    }
    sm[threadIdx.x] = bad ? NAN : m; sc[threadIdx.x] = cnt; si[threadIdx.x] = it;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double a = sm[threadIdx.x], b = sm[threadIdx.x + o];
            sm[threadIdx.x] = (a != a || b != b) ? NAN : fmax(a, b);
            sc[threadIdx.x] += sc[threadIdx.x + o];
            si[threadIdx.x] = fmax(si[threadIdx.x], si[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = sm[0]; out[1] = sc[0]; out[2] = si[0]; }
}

// ---- replace_nan_with_channel_mean ----------------------------------------------------------------------------------------------
// blockDim = (64 channels, 4 pixel groups); slice blockIdx.y of the pixels, every thread in ascending pixel order:
// partial[(slice 4 + group)][c] = (sum, count) over the voxels of channel c that are not NaN
template <typename T>
__global__ __launch_bounds__(256) void k_nan_partial(const T* __restrict__ cube, long long npix, int N, double* __restrict__ psum,
                                                     double* __restrict__ pcnt) {
    const int c = blockIdx.x * 64 + threadIdx.x, grp = threadIdx.y;
    if (c >= N) return;
    const long long per = (npix + gridDim.y - 1) / gridDim.y;
    const long long p0 = (long long)blockIdx.y * per, p1 = p0 + per < npix ? p0 + per : npix;
    double s = 0.0, n = 0.0;
    for (long long p = p0 + grp; p < p1; p += 4) {
        const double v = (double)cube[p * N + c];
        if (v == v) { s += v; n += 1.0; }
    }
    const size_t o = ((size_t)blockIdx.y * 4 + grp) * N + c;
    psum[o] = s; pcnt[o] = n;
}
// mean[c] = sum / count in partial order (NaN for a channel without a finite voxel)
__global__ __launch_bounds__(256) void k_nan_mean(const double* __restrict__ psum, const double* __restrict__ pcnt, int nrows, int N,
                                                  double* __restrict__ mean) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    double s = 0.0, n = 0.0;
    for (int q = 0; q < nrows; ++q) { s += psum[(size_t)q * N + c]; n += pcnt[(size_t)q * N + c]; }
    mean[c] = n > 0.0 ? s / n : NAN;
}
// a voxel that is not NaN is copied bit for bit
template <typename T>
__global__ __launch_bounds__(256) void k_nan_replace(const T* __restrict__ cube, const double* __restrict__ mean, T* __restrict__ out,
                                                     long long n, int N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const T v = cube[i];
        out[i] = v == v ? v : (T)mean[i % N];
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
int elem_blocks(const fb_plan* p, long long n) {
    const long long b = (n + 255) / 256, cap = 16LL * p->num_cu;
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}
fb::RngKey make_key(uint64_t seed, uint64_t real) {
    fb::RngKey k;
    k.k[0] = (uint32_t)seed; k.k[1] = (uint32_t)(seed >> 32); k.k[2] = (uint32_t)real; k.k[3] = (uint32_t)(real >> 32);
    return k;
}

template <typename TX>
int los_matmul(fb_plan* p, const double* M, const void* X, const double* pre, const double* post, const double* add, double* Y,
               hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    const dim3 grid((unsigned)((npix + 32 * FB_LOS_MP - 1) / (32 * FB_LOS_MP)), (unsigned)((N + 32 * FB_LOS_MC - 1) / (32 * FB_LOS_MC)));
    const bool edge = N % (16 * FB_LOS_MC) != 0 || npix % (32 * FB_LOS_MP) != 0;
    FbProfScope _ps(p, FBK_PCA, s);
    if (edge) hipLaunchKernelGGL((k_los_matmul<TX, true>), grid, dim3(256), 0, s, M, (const TX*)X, pre, post, add, Y, npix, N);
    else hipLaunchKernelGGL((k_los_matmul<TX, false>), grid, dim3(256), 0, s, M, (const TX*)X, pre, post, add, Y, npix, N);
    FB_LAUNCH_CHECK("k_los_matmul");
    return FB_OK;
}
int los_matmul_kind(fb_plan* p, const double* M, const void* X, int x_kind, const double* pre, const double* post, const double* add,
                    double* Y, hipStream_t s) {
    if (x_kind == FB_LOS_X_FP64 || p->prec == 8) return los_matmul<double>(p, M, X, pre, post, add, Y, s);
    return los_matmul<float>(p, M, X, pre, post, add, Y, s);
}

// A v = v + S^(1/2) (q (S^(1/2) v)), t = scratch
int apply_A(fb_plan* p, const double* sqrtS, const double* q, const double* v, double* t, double* out, hipStream_t s) {
    int r = los_matmul<double>(p, sqrtS, v, nullptr, q, nullptr, t, s);
    if (r) return r;
    return los_matmul<double>(p, sqrtS, t, nullptr, nullptr, v, out, s);
}

template <typename T>
int gcr_rhs(fb_plan* p, const void* d, const void* w, int w_kind, const void* var, int var_kind, const double* omega2, int draws,
            uint64_t seed, uint64_t real, double* q, double* u, double* omega1_out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_gcr_rhs<T>), dim3(elem_blocks(p, n)), dim3(256), 0, s, (const T*)d, w, w_kind, var, var_kind, omega2, draws,
                       make_key(seed, real), q, u, omega1_out, n, p->N);
    FB_LAUNCH_CHECK("k_gcr_rhs");
    return FB_OK;
}

template <typename T>
int gcr_finish(fb_plan* p, const double* sv, const void* var, int var_kind, const double* omega3, int noise, uint64_t seed,
               uint64_t real, const void* d, const void* w, int w_kind, int inpaint, void* out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_gcr_finish<T>), dim3(elem_blocks(p, n)), dim3(256), 0, s, sv, var, var_kind, omega3, noise,
                       make_key(seed, real), (const T*)d, w, w_kind, inpaint, (T*)out, n, p->N);
    FB_LAUNCH_CHECK("k_gcr_finish");
    return FB_OK;
}

template <typename T>
int replace_nan(fb_plan* p, const void* cube, void* out, double* mean_out, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N, n = npix * N;
    int slices = (int)((npix + 255) / 256);
    if (slices > 256) slices = 256;
    const int nrows = 4 * slices;
    // work: [mean: N | sums: nrows N | counts: nrows N]
    FB_TRY(p->work.ensure((size_t)(1 + 2 * nrows) * N * sizeof(double)));
    double* mean = p->work.as<double>();
    double* psum = mean + N;
    double* pcnt = psum + (size_t)nrows * N;
    FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL((k_nan_partial<T>), dim3((N + 63) / 64, slices), dim3(64, 4), 0, s, (const T*)cube, npix, N, psum, pcnt);
    hipLaunchKernelGGL(k_nan_mean, dim3((N + 255) / 256), dim3(256), 0, s, (const double*)psum, (const double*)pcnt, nrows, N, mean);
    hipLaunchKernelGGL((k_nan_replace<T>), dim3(elem_blocks(p, n)), dim3(256), 0, s, (const T*)cube, (const double*)mean, (T*)out, n, N);
    FB_LAUNCH_CHECK("k_nan_replace");
    if (mean_out) FB_HIP(hipMemcpyAsync(mean_out, mean, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_los_matmul(fb_plan* p, const double* M_dev, const void* X, int x_kind, const double* pre, const double* post,
                  const double* add, double* Y, void* stream) {
    FB_REQUIRE(p && M_dev && X && Y, "null pointer");
    FB_REQUIRE(x_kind == FB_LOS_X_PLAN || x_kind == FB_LOS_X_FP64, "x_kind: FB_LOS_X_PLAN or FB_LOS_X_FP64");
    FB_REQUIRE((const void*)Y != X && (const void*)Y != (const void*)pre, "fb_los_matmul: Y must not be X or pre");
    FB_REQUIRE(p->N <= FB_GCR_NMAX, "fb_los_matmul: at most 1024 channels");
    FB_USE_DEVICE(p);
    return los_matmul_kind(p, M_dev, X, x_kind, pre, post, add, Y, (hipStream_t)stream);
}

int fb_gcr_rhs(fb_plan* p, const void* d, const void* w, int w_kind, const void* var, int var_kind, const double* omega2, int draws,
               uint64_t seed, uint64_t realisation, double* q_out, double* u_out, double* omega1_out, double* qmean_dev, void* stream) {
    FB_REQUIRE(p && d && w && var && q_out && u_out, "null pointer");
    FB_REQUIRE((w_kind == FB_GCR_PER_CHANNEL || w_kind == FB_GCR_PER_VOXEL) && (var_kind == FB_GCR_PER_CHANNEL || var_kind == FB_GCR_PER_VOXEL),
               "w_kind, var_kind: FB_GCR_PER_CHANNEL or FB_GCR_PER_VOXEL");
    FB_REQUIRE(draws == FB_GCR_DRAWS_NONE || (draws == FB_GCR_DRAWS_GIVEN && omega2) || (draws == FB_GCR_DRAWS_DEVICE && omega1_out),
               "draws: FB_GCR_DRAWS_NONE, _GIVEN with omega2, or _DEVICE with omega1_out");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const int r = FB_DISPATCH(p, gcr_rhs<float>(p, d, w, w_kind, var, var_kind, omega2, draws, seed, realisation, q_out, u_out, omega1_out, s),
                              gcr_rhs<double>(p, d, w, w_kind, var, var_kind, omega2, draws, seed, realisation, q_out, u_out, omega1_out, s));
    if (r || !qmean_dev) return r;
    return fbi_channel_means_f64(p, q_out, qmean_dev, s);          // q is fp64 whatever the plan: the fp64 instance serves both
}

int fb_gcr_solve(fb_plan* p, const double* sqrtS_dev, const double* P_dev, const double* q, const double* b, double* x, double* work,
                 double tol, int maxiter, int32_t* n_iter_dev, double* info_out, void* stream) {
    FB_REQUIRE(p && sqrtS_dev && q && b && x && work && n_iter_dev && info_out, "null pointer");
    FB_REQUIRE(tol > 0.0 && maxiter >= 1, "fb_gcr_solve: tol > 0 and maxiter >= 1");
    FB_REQUIRE(p->N <= FB_GCR_NMAX, "fb_gcr_solve: at most 1024 channels");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const int N = p->N;
    const long long npix = (long long)N * N;
    const size_t n = (size_t)npix * N;
    double* r = work;
    double* pd = work + n;
    double* ap = work + 2 * n;
    double* t = work + 3 * n;
    double* z = P_dev ? work + 4 * n : r;                 // without a preconditioner z is r itself
    // row state: [rz | bb | res: npix doubles each | summary: 4 | active: npix ints | count: 2 ints]
    int rc = p->work.ensure((size_t)npix * (3 * sizeof(double) + sizeof(int)) + 4 * sizeof(double) + 2 * sizeof(int));
    if (rc) return rc;
    GcrRows st;
    st.rz = p->work.as<double>();
    st.bb = st.rz + npix;
    double* res = st.bb + npix;
    double* summary = res + npix;
    st.active = (int*)(summary + 4);
    st.count = st.active + npix;
    st.n_iter = n_iter_dev;
    const dim3 rows((unsigned)((npix + 3) / 4));
    int active = 0;
    FB_HIP(hipMemsetAsync(st.count, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_cg_init, rows, dim3(256), 0, s, b, x, r, st, npix, N);
    FB_LAUNCH_CHECK("k_cg_init");
    FB_TRY(fb_read_back(&active, st.count, sizeof(int), s));
    int it = 0;
    for (; active > 0 && it < maxiter; ++it) {
        if (P_dev) { rc = los_matmul<double>(p, P_dev, r, nullptr, nullptr, nullptr, z, s); if (rc) return rc; }
        hipLaunchKernelGGL(k_cg_direction, rows, dim3(256), 0, s, (const double*)r, (const double*)z, pd, st, it == 0 ? 1 : 0, npix, N);
        rc = apply_A(p, sqrtS_dev, q, pd, t, ap, s);
        if (rc) return rc;
        FB_HIP(hipMemsetAsync(st.count, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_cg_step, rows, dim3(256), 0, s, (const double*)pd, (const double*)ap, x, r, st, tol * tol, npix, N);
        FB_LAUNCH_CHECK("k_cg_step");
        FB_TRY(fb_read_back(&active, st.count, sizeof(int), s));
    }
    // the true residual, from one more application of A
    rc = apply_A(p, sqrtS_dev, q, x, t, ap, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_row_residual, rows, dim3(256), 0, s, b, (const double*)ap, st, res, npix, N);
    hipLaunchKernelGGL(k_gcr_summary, dim3(1), dim3(1024), 0, s, (const double*)res, (const int32_t*)n_iter_dev, (const int*)st.active, npix, summary);
    FB_LAUNCH_CHECK("k_gcr_summary");
    double h[3];
    FB_TRY(fb_read_back(h, summary, sizeof(h), s));
    info_out[0] = h[0]; info_out[1] = h[1]; info_out[2] = h[2]; info_out[3] = (double)it;
    return FB_OK;
}

int fb_gcr_finish(fb_plan* p, const double* sqrtS_dev, const double* x, double* s_work, const void* var, int var_kind,
                  const double* omega3, int noise, uint64_t seed, uint64_t realisation, const void* d, const void* w, int w_kind,
                  int inpaint, void* out, void* stream) {
    FB_REQUIRE(p && sqrtS_dev && x && s_work && out, "null pointer");
    FB_REQUIRE(s_work != x, "fb_gcr_finish: s_work must not be x");
    FB_REQUIRE(noise == FB_GCR_DRAWS_NONE || (var && (noise == FB_GCR_DRAWS_DEVICE || (noise == FB_GCR_DRAWS_GIVEN && omega3))),
               "noise: FB_GCR_DRAWS_NONE, or a variance with _GIVEN and omega3 or _DEVICE");
    FB_REQUIRE(!inpaint || (d && w), "in-painting needs d and w");
    FB_REQUIRE((w_kind == FB_GCR_PER_CHANNEL || w_kind == FB_GCR_PER_VOXEL) && (var_kind == FB_GCR_PER_CHANNEL || var_kind == FB_GCR_PER_VOXEL),
               "w_kind, var_kind: FB_GCR_PER_CHANNEL or FB_GCR_PER_VOXEL");
    FB_REQUIRE(p->N <= FB_GCR_NMAX, "fb_gcr_finish: at most 1024 channels");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    int rc = los_matmul<double>(p, sqrtS_dev, x, nullptr, nullptr, nullptr, s_work, s);
    if (rc) return rc;
    return FB_DISPATCH(p, gcr_finish<float>(p, s_work, var, var_kind, omega3, noise, seed, realisation, d, w, w_kind, inpaint, out, s),
                       gcr_finish<double>(p, s_work, var, var_kind, omega3, noise, seed, realisation, d, w, w_kind, inpaint, out, s));
}

int fb_replace_nan_channel_mean(fb_plan* p, const void* cube, void* cube_out, double* mean_dev, void* stream) {
    FB_REQUIRE(p && cube && cube_out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, replace_nan<float>(p, cube, cube_out, mean_dev, s), replace_nan<double>(p, cube, cube_out, mean_dev, s));
}

}  // extern "C"
