// Density-field (BAO) reconstruction and mesh readout (CosmoBox.reconstruct, .readout, .uniform_catalogue; defined by this
// project -- Eisenstein et al. 2007, Padmanabhan et al. 2012, Burden et al. 2014 -- in DESIGN.md section 4 and stated in numpy
// in tests/recon_numpy.py): the smoothed, bias- and beta-weighted displacement of a density, the readout of up to three real
// fields at particle positions through fb_paint's windows, the same fused with the shift of the particles, and uniform random
// positions.  Both plan precisions are compiled here; see include/fastbox_hip.h for the entry points.
//
// Particle data are fp64 whatever the plan's precision, and so is all arithmetic; the fields are read in the plan's precision.
// No contraction: the numpy statement rounds every operation once, in the order written here.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include "fb_rng.h"
#include <cmath>

#define FB_RECON_STAGE_DIV 8              // fb_recon_shift stages Psi interleaved for n >= N^3 / 8 particles (see shift<>)
#define FB_RECON_STREAM 10u              // Philox stream of fb_uniform_positions (0-9: fb_rng.h, fb_halo.hip, fb_inpaint.hip)

namespace {
using namespace fb;

constexpr double kTwoPi = 6.283185307179586;     // the double 2 * np.pi

// Psi_a(k) = i k_a delta(k) exp(-k^2 R^2 / 2) / (b (k^2 + beta k_z^2)) for a = x, y, z in one pass over delta(k): one read, three
// half spectra written.  k_a = 2 pi m_a / L_a with m_a the signed index (N/2 -> -N/2); zero at k = 0; component a is zero on
// the plane m_a = -N/2 (k_cola_kmul's convention); the padding of the half-spectrum layout is zeroed.
template <typename T>
__global__ __launch_bounds__(256) void k_recon_kmul(const T* __restrict__ in, T* __restrict__ ox, T* __restrict__ oy,
                                                    T* __restrict__ oz, int N, int NR, int NZP, double L0, double L1, double L2,
                                                    double RR, double b, double beta) {
    const int NZV = N / 2 + 1;
    const unsigned long long n = (unsigned long long)N * NR * NZP;
    T* const out[3] = {ox, oy, oz};
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256) {
        const unsigned long long row = q / (unsigned)NZP;
        const int l = (int)(q - row * (unsigned)NZP), j = (int)(row % (unsigned)NR), i = (int)(row / (unsigned)NR);
        double r[3] = {0.0, 0.0, 0.0}, re = 0.0, im = 0.0;
        if (l < NZV && j < N) {
            const int m[3] = {mode_of(i, N), mode_of(j, N), mode_of(l, N)};
            const double k[3] = {(kTwoPi * m[0]) / L0, (kTwoPi * m[1]) / L1, (kTwoPi * m[2]) / L2};
            const double kz2 = k[2] * k[2], kk = (k[0] * k[0] + k[1] * k[1]) + kz2;
            if (kk != 0.0) {
                const double c = exp(-0.5 * (kk * RR)) / (b * (kk + beta * kz2));
                for (int a = 0; a < 3; ++a)
                    if (m[a] != -(N / 2)) r[a] = k[a] * c;
            }
            re = (double)in[2 * q]; im = (double)in[2 * q + 1];
        }
        for (int a = 0; a < 3; ++a) {
            out[a][2 * q] = (T)(-(r[a] * im));
            out[a][2 * q + 1] = (T)(r[a] * re);
        }
    }
}

// sum over the window's nodes of w F at u (cells), for NF fields read as T -- [NF][nv], or with IL (x, y, z, pad) per node; W: 0
// ngp, 1 cic, 2 tsc (W + 1 nodes an axis).  The order of the sum is the statement's: x outermost, the weight ((w_x w_y) w_z).
template <typename T> struct alignas(4 * sizeof(T)) Vec4 { T v[4]; };
template <typename T, int NF, int W, bool IL = false>
__device__ __forceinline__ void gather(const T* __restrict__ F, unsigned long long nv, int N, const double (&u)[3],
                                       double (&g)[NF]) {
    constexpr int NW = W + 1;
    long long m[3][3];
    double w[3][3];
    for (int c = 0; c < 3; ++c) (void)axis_weights(u[c], W, N, m[c], w[c]);
    for (int c = 0; c < NF; ++c) g[c] = 0.0;
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const unsigned long long row = ((unsigned long long)m[0][a] * N + (unsigned long long)m[1][b]) * N;
            const double wab = w[0][a] * w[1][b];
#pragma unroll
            for (int e = 0; e < NW; ++e) {
                const double wt = wab * w[2][e];
                const unsigned long long node = row + (unsigned long long)m[2][e];
                if (IL) {                         // (x, y, z, pad) per node: one load
                    const Vec4<T> q = reinterpret_cast<const Vec4<T>*>(F)[node];
#pragma unroll
                    for (int c = 0; c < NF; ++c) g[c] += wt * (double)q.v[c];
                } else {
#pragma unroll
                    for (int c = 0; c < NF; ++c) g[c] += wt * (double)F[c * nv + node];
                }
            }
        }
}
__device__ __forceinline__ bool finite3(double x0, double x1, double x2) {
    return fabs(x0) < 1e300 && fabs(x1) < 1e300 && fabs(x2) < 1e300;
}

// out[i][c] = readout of field c at particle i; lanes take consecutive particles.  A position that is not finite reads NaN.
template <typename T, int NF, int W>
__global__ __launch_bounds__(256) void k_mesh_readout(const T* __restrict__ F, unsigned long long nv, int N,
                                                      const double* __restrict__ pos, unsigned long long n, double s0, double s1,
                                                      double s2, double* __restrict__ out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double x0 = pos[3 * i], x1 = pos[3 * i + 1], x2 = pos[3 * i + 2];
        double g[NF];
        if (finite3(x0, x1, x2)) {
            const double u[3] = {x0 * s0, x1 * s1, x2 * s2};
            gather<T, NF, W>(F, nv, N, u, g);
        } else {
            for (int c = 0; c < NF; ++c) g[c] = __builtin_nan("");
        }
        for (int c = 0; c < NF; ++c) out[(unsigned long long)NF * i + c] = g[c];
    }
}

// pos_out = wrap(x - scale Psi(x) - scale_z Psi_z(x) z^): the readout of psi [3][nv] fused with the shift.  pos_out may be
// pos_in: a lane reads its particle before it writes it, and no lane reads another's.
template <typename T, int W, bool IL>
__global__ __launch_bounds__(256) void k_recon_shift(const T* __restrict__ psi, unsigned long long nv, int N, const double* pos_in,
                                                     unsigned long long n, double s0, double s1, double s2, double L0, double L1,
                                                     double L2, double scale, double scale_z, double* pos_out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double x0 = pos_in[3 * i], x1 = pos_in[3 * i + 1], x2 = pos_in[3 * i + 2];
        double r0, r1, r2;
        r0 = r1 = r2 = __builtin_nan("");
        if (finite3(x0, x1, x2)) {
            const double u[3] = {x0 * s0, x1 * s1, x2 * s2};
            double g[3];
            gather<T, 3, W, IL>(psi, nv, N, u, g);
            r0 = wrap_pos(x0 - scale * g[0], L0);
            r1 = wrap_pos(x1 - scale * g[1], L1);
            r2 = wrap_pos(x2 - (scale * g[2] + scale_z * g[2]), L2);
        }
        pos_out[3 * i] = r0; pos_out[3 * i + 1] = r1; pos_out[3 * i + 2] = r2;
    }
}

// psi4[node] = (Psi_x, Psi_y, Psi_z, 0)[node] from psi3 [3][nv]
template <typename T>
__global__ __launch_bounds__(256) void k_recon_interleave(const T* __restrict__ psi3, unsigned long long nv, Vec4<T>* __restrict__ out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (unsigned long long)gridDim.x * 256) {
        Vec4<T> q;
        q.v[0] = psi3[i]; q.v[1] = psi3[nv + i]; q.v[2] = psi3[2 * nv + i]; q.v[3] = T(0);
        out[i] = q;
    }
}

// Point p: calls 2 p and 2 p + 1 of the stream (one call holds 128 bits, three 53-bit uniforms take 159).  x from words (0, 1)
// and y from words (2, 3) of call 2 p, z from words (0, 1) of call 2 p + 1; each u = (w + 1/2) 2^-53 with w = (a << 21) | (b >> 11)
// (fb_halo.hip's poisson_uniform), times L_a, and no larger than the largest double below L_a (w + 1/2 rounds to 2^53 for the
// last w).  Host model: fastbox_amd/rng.py recon_uniforms.
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {
    const unsigned long long w = ((unsigned long long)a << 21) | (unsigned long long)(b >> 11);
    return ((double)w + 0.5) * 1.1102230246251565e-16;
}
__global__ __launch_bounds__(256) void k_uniform_positions(RngKey key, unsigned long long n, double L0, double L1, double L2,
                                                           double M0, double M1, double M2, double* __restrict__ pos) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        uint32_t X[2][4];
        philox_counter(2 * i, FB_RECON_STREAM, key, X[0]);
        philox_counter(2 * i + 1, FB_RECON_STREAM, key, X[1]);
        philox4x32_batch<2>(X, key.k[0], key.k[1]);
        pos[3 * i] = fmin(uniform53(X[0][0], X[0][1]) * L0, M0);
        pos[3 * i + 1] = fmin(uniform53(X[0][2], X[0][3]) * L1, M1);
        pos[3 * i + 2] = fmin(uniform53(X[1][0], X[1][1]) * L2, M2);
    }
}

// one particle on each mesh node, C order: node (i, j, l) at (i h_x, j h_y, l h_z)
__global__ __launch_bounds__(256) void k_grid_positions(unsigned long long nv, int N, double h0, double h1, double h2,
                                                        double* __restrict__ pos) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long row = i / (unsigned)N;
        pos[3 * i] = (double)(row / (unsigned)N) * h0;
        pos[3 * i + 1] = (double)(row % (unsigned)N) * h1;
        pos[3 * i + 2] = (double)(i - row * (unsigned)N) * h2;
    }
}

unsigned long long nv_of(const fb_plan* p) { return (unsigned long long)p->N * p->N * p->N; }

template <typename T>
int displacement(fb_plan* p, const void* half_in, void* half_work3, void* psi3, double R, double b, double beta, hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->NR * p->NZP, nv = nv_of(p);
    T* h[3] = {(T*)half_work3, (T*)half_work3 + 2 * n, (T*)half_work3 + 4 * n};
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_recon_kmul<T>), dim3(grid_for(n, p)), dim3(256), 0, s, (const T*)half_in, h[0], h[1], h[2], p->N, p->NR,
                       p->NZP, p->L[0], p->L[1], p->L[2], R * R, b, beta); }
    FB_LAUNCH_CHECK("k_recon_kmul");
    const double sc = 1.0 / (double)nv;
    for (int c = 0; c < 3; ++c)
        FB_TRY(sizeof(T) == 4 ? fbi_fft_c2r_f32(p, h[c], (T*)psi3 + c * nv, sc, s) : fbi_fft_c2r_f64(p, h[c], (T*)psi3 + c * nv, sc, s));
    return FB_OK;
}

template <typename T, int NF>
int readout_w(fb_plan* p, const T* F, const double* pos, unsigned long long n, int window, double* out, hipStream_t s) {
    const unsigned long long nv = nv_of(p);
    const double s0 = (double)p->N / p->L[0], s1 = (double)p->N / p->L[1], s2 = (double)p->N / p->L[2];
    const dim3 g(grid_for(n, p)), blk(256);
    FbProfScope _ps(p, FBK_REALOP, s);
    if (window == FB_WINDOW_NGP) hipLaunchKernelGGL((k_mesh_readout<T, NF, 0>), g, blk, 0, s, F, nv, p->N, pos, n, s0, s1, s2, out);
    else if (window == FB_WINDOW_CIC) hipLaunchKernelGGL((k_mesh_readout<T, NF, 1>), g, blk, 0, s, F, nv, p->N, pos, n, s0, s1, s2, out);
    else hipLaunchKernelGGL((k_mesh_readout<T, NF, 2>), g, blk, 0, s, F, nv, p->N, pos, n, s0, s1, s2, out);
    return FB_OK;
}
template <typename T>
int readout(fb_plan* p, const void* fields, int nf, const double* pos, unsigned long long n, int window, double* out, hipStream_t s) {
    if (nf == 1) FB_TRY((readout_w<T, 1>(p, (const T*)fields, pos, n, window, out, s)));
    else if (nf == 2) FB_TRY((readout_w<T, 2>(p, (const T*)fields, pos, n, window, out, s)));
    else FB_TRY((readout_w<T, 3>(p, (const T*)fields, pos, n, window, out, s)));
    FB_LAUNCH_CHECK("k_mesh_readout");
    return FB_OK;
}

template <typename T, bool IL>
void launch_shift(const T* psi, unsigned long long nv, fb_plan* p, const double* pos_in, unsigned long long n, int window, double scale,
                  double scale_z, double* pos_out, hipStream_t s) {
    const double s0 = (double)p->N / p->L[0], s1 = (double)p->N / p->L[1], s2 = (double)p->N / p->L[2];
    const dim3 g(grid_for(n, p)), blk(256);
    if (window == FB_WINDOW_NGP)
        hipLaunchKernelGGL((k_recon_shift<T, 0, IL>), g, blk, 0, s, psi, nv, p->N, pos_in, n, s0, s1, s2, p->L[0], p->L[1], p->L[2], scale,
                           scale_z, pos_out);
    else if (window == FB_WINDOW_CIC)
        hipLaunchKernelGGL((k_recon_shift<T, 1, IL>), g, blk, 0, s, psi, nv, p->N, pos_in, n, s0, s1, s2, p->L[0], p->L[1], p->L[2], scale,
                           scale_z, pos_out);
    else
        hipLaunchKernelGGL((k_recon_shift<T, 2, IL>), g, blk, 0, s, psi, nv, p->N, pos_in, n, s0, s1, s2, p->L[0], p->L[1], p->L[2], scale,
                           scale_z, pos_out);
}
// Catalogues of at least nv / FB_RECON_STAGE_DIV particles read Psi from an interleaved copy (x, y, z, pad per node, staged into
// the plan's shared work buffer): one load per node instead of three, in three distant rows.  Measured: the
// copy costs 5 ps per node, the interleaved gather saves 40 ps per particle in COLA order and 165 ps shuffled -- the break-even
// is n = nv / 8 for ordered particles.  Both forms add the same products in the same order: the same bits.
template <typename T>
int shift(fb_plan* p, const void* psi3, const double* pos_in, unsigned long long n, int window, double scale, double scale_z,
          double* pos_out, hipStream_t s) {
    const unsigned long long nv = nv_of(p);
    if (n >= nv / FB_RECON_STAGE_DIV) {
        FB_TRY(p->work.ensure(nv * sizeof(Vec4<T>)));
        Vec4<T>* psi4 = p->work.as<Vec4<T>>();
        { FbProfScope _ps(p, FBK_LAYOUT, s);
        hipLaunchKernelGGL((k_recon_interleave<T>), dim3(grid_for(nv, p)), dim3(256), 0, s, (const T*)psi3, nv, psi4); }
        FB_LAUNCH_CHECK("k_recon_interleave");
        FbProfScope _ps(p, FBK_REALOP, s);
        launch_shift<T, true>((const T*)psi4, nv, p, pos_in, n, window, scale, scale_z, pos_out, s);
    } else {
        FbProfScope _ps(p, FBK_REALOP, s);
        launch_shift<T, false>((const T*)psi3, nv, p, pos_in, n, window, scale, scale_z, pos_out, s);
    }
    FB_LAUNCH_CHECK("k_recon_shift");
    return FB_OK;
}

int catalogue_check(const fb_plan* p, int64_t n, int window) {
    FB_REQUIRE(n >= 0 && n <= 2147483646ll, "n must be between 0 and 2^31 - 2");
    FB_REQUIRE(window >= FB_WINDOW_NGP && window <= FB_WINDOW_TSC, "window must be FB_WINDOW_NGP, _CIC or _TSC");
    FB_REQUIRE(!p->comm, "reconstruction and mesh readout run on a single-GPU plan");
    return FB_OK;
}

}  // namespace

extern "C" {

int64_t fb_recon_work_bytes(const fb_plan* p, int64_t n_data, int64_t n_random) {
    if (!p || n_data < 0 || n_random < 0) return -1;
    const int64_t real = fb_real_bytes(p), half = fb_half_bytes(p);
    // delta, D, S, delta_rec, Psi[3] and its interleaved copy; delta(k) and the three work spectra; the shifted catalogues;
    // fb_paint's accumulators
    return 11 * real + 4 * half + 24 * (n_data + n_random) + (int64_t)nv_of(p) * 8 * (p->prec == 8 ? 2 : 1) + (1 << 16);
}

int fb_recon_displacement(fb_plan* p, const void* half_in, void* half_work3, void* psi3_out, double R, double b, double beta,
                          void* stream) {
    FB_REQUIRE(p && half_in && half_work3 && psi3_out, "null pointer");
    FB_REQUIRE(R > 0.0 && R < 1e150 && b > 0.0 && b < 1e300 && beta >= 0.0 && beta < 1e300,
               "smoothing and bias must be positive and beta >= 0, all finite");
    FB_REQUIRE(!p->comm, "reconstruction and mesh readout run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, displacement<float>(p, half_in, half_work3, psi3_out, R, b, beta, s),
                       displacement<double>(p, half_in, half_work3, psi3_out, R, b, beta, s));
}

int fb_mesh_readout(fb_plan* p, const void* fields, int nfields, const double* pos, int64_t n, int window, double* out,
                    void* stream) {
    FB_REQUIRE(p && fields, "null pointer");
    FB_REQUIRE(nfields >= 1 && nfields <= 3, "nfields must be 1, 2 or 3");
    int r = catalogue_check(p, n, window);
    if (r) return r;
    if (n == 0) return FB_OK;
    FB_REQUIRE(pos && out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, readout<float>(p, fields, nfields, pos, (unsigned long long)n, window, out, s),
                       readout<double>(p, fields, nfields, pos, (unsigned long long)n, window, out, s));
}

int fb_recon_shift(fb_plan* p, const void* psi3, const double* pos_in, int64_t n, int window, double scale, double scale_z,
                   double* pos_out, void* stream) {
    FB_REQUIRE(p && psi3, "null pointer");
    FB_REQUIRE(fabs(scale) < 1e300 && fabs(scale_z) < 1e300, "scale and scale_z must be finite");
    int r = catalogue_check(p, n, window);
    if (r) return r;
    if (n == 0) return FB_OK;
    FB_REQUIRE(pos_in && pos_out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, shift<float>(p, psi3, pos_in, (unsigned long long)n, window, scale, scale_z, pos_out, s),
                       shift<double>(p, psi3, pos_in, (unsigned long long)n, window, scale, scale_z, pos_out, s));
}

int fb_uniform_positions(fb_plan* p, uint64_t seed, uint64_t realisation, int64_t n, double* pos_out, void* stream) {
    FB_REQUIRE(p, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll, "n must be between 0 and 2^31 - 2");
    if (n == 0) return FB_OK;
    FB_REQUIRE(pos_out, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    RngKey k;
    k.k[0] = (uint32_t)seed; k.k[1] = (uint32_t)(seed >> 32); k.k[2] = (uint32_t)realisation; k.k[3] = (uint32_t)(realisation >> 32);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_uniform_positions, dim3(grid_for((unsigned long long)n, p)), dim3(256), 0, s, k, (unsigned long long)n,
                       p->L[0], p->L[1], p->L[2], std::nextafter(p->L[0], 0.0), std::nextafter(p->L[1], 0.0),
                       std::nextafter(p->L[2], 0.0), pos_out); }
    FB_LAUNCH_CHECK("k_uniform_positions");
    return FB_OK;
}

int fb_grid_positions(fb_plan* p, double* pos_out, void* stream) {
    FB_REQUIRE(p && pos_out, "null pointer");
    FB_REQUIRE(nv_of(p) <= 2147483646ull, "at most 2^31 - 2 nodes");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_grid_positions, dim3(grid_for(nv_of(p), p)), dim3(256), 0, s, nv_of(p), p->N, p->L[0] / (double)p->N,
                       p->L[1] / (double)p->N, p->L[2] / (double)p->N, pos_out); }
    FB_LAUNCH_CHECK("k_grid_positions");
    return FB_OK;
}

}  // extern "C"
