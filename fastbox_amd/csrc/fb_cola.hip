// COLA particle-mesh (CosmoBox.realise_density_cola; the reference's fastbox/box.py:463-589 hands this to pycola3): 2LPT
// displacements, the PM force, the COLA kick/drift and the particles' velocities on the mesh.  Both plan precisions are
// compiled here; see include/fastbox_hip.h for the entry points and DESIGN.md section 4 for the definition.
//
// Particle i starts on node i (C order, node m at m L / N: fb_paint's convention), so a real field of the plan's precision
// doubles as a per-particle array: Psi1, Psi2, p_res and the force are [3][N^3] blocks indexed by particle.  Positions are
// fp64 [N^3][3] (what fb_paint reads).  No contraction: the numpy statement of the definition (tests/cola_numpy.py) rounds
// every operation once, in the order written here.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <algorithm>
#include <cmath>

namespace {
using namespace fb;

constexpr double kTwoPi = 6.283185307179586;     // the double 2 * np.pi

// N/2 -> -N/2 (fftfreq).  For N >= 0 these are the values of mode_of (fb_dev.h); it stays here, written with the `N / 2` that
// k_cola_kmul's plane tests (m == -N / 2) use, so that the convention and its tests read as one.  The mode that does differ
// is k_paint_compensate's (fb_halo.hip): it keeps +N/2.
__device__ __forceinline__ int signed_mode(int i, int N) { return i < N / 2 ? i : i - N; }

// out = c * in on a half spectrum: b < 0: c i k_a / k^2 (zero at k = 0 and on the plane m_a = -N/2);
// b >= 0: c k_a k_b / k^2 (zero at k = 0; for a != b also on the planes m_a = -N/2 and m_b = -N/2).  k_a = 2 pi m_a / L.
template <typename T>
__global__ __launch_bounds__(256) void k_cola_kmul(const T* __restrict__ in, T* __restrict__ out, int N, int NR, int NZP,
                                                   double L, int a, int b, double c) {
    const int NZV = N / 2 + 1;
    const unsigned long long n = (unsigned long long)N * NR * NZP;
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256) {
        const unsigned long long row = q / (unsigned)NZP;
        const int l = (int)(q - row * (unsigned)NZP), j = (int)(row % (unsigned)NR), i = (int)(row / (unsigned)NR);
        if (l >= NZV || j >= N) { out[2 * q] = T(0); out[2 * q + 1] = T(0); continue; }
        const int m[3] = {signed_mode(i, N), signed_mode(j, N), signed_mode(l, N)};
        const double k0 = (kTwoPi * m[0]) / L, k1 = (kTwoPi * m[1]) / L, k2 = (kTwoPi * m[2]) / L;
        const double kk = (k0 * k0 + k1 * k1) + k2 * k2;
        const double ka = a == 0 ? k0 : (a == 1 ? k1 : k2);
        const double re = (double)in[2 * q], im = (double)in[2 * q + 1];
        double r = 0.0;
        if (b < 0) {
            if (kk != 0.0 && m[a] != -N / 2) r = (c * ka) / kk;
            out[2 * q] = (T)(-(r * im));
            out[2 * q + 1] = (T)(r * re);
        } else {
            const double kb = b == 0 ? k0 : (b == 1 ? k1 : k2);
            if (kk != 0.0 && (a == b || (m[a] != -N / 2 && m[b] != -N / 2))) r = (c * (ka * kb)) / kk;
            out[2 * q] = (T)(r * re);
            out[2 * q + 1] = (T)(r * im);
        }
    }
}

// 2LPT source in one pass over the six second derivatives: d = [xx, yy, zz], o = [xy, xz, yz] ([3][N^3] each); S over o[0]
template <typename T>
__global__ __launch_bounds__(256) void k_cola_source(const T* __restrict__ d, T* __restrict__ o, unsigned long long n3) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256) {
        const double xx = d[i], yy = d[n3 + i], zz = d[2 * n3 + i];
        const double xy = o[i], xz = o[n3 + i], yz = o[2 * n3 + i];
        const double s = ((((xx * yy + xx * zz) + yy * zz) - xy * xy) - xz * xz) - yz * yz;
        o[i] = (T)s;
    }
}

// pos = wrap(q + d1 Psi1 + d2 Psi2); p_res = 0
template <typename T>
__global__ __launch_bounds__(256) void k_cola_init(const T* __restrict__ psi1, const T* __restrict__ psi2, unsigned long long n3,
                                                   int N, double cell, double L, double d1, double d2, double* __restrict__ pos,
                                                   T* __restrict__ pres) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long row = i / (unsigned)N;
        const int m[3] = {(int)(row / (unsigned)N), (int)(row % (unsigned)N), (int)(i - row * (unsigned)N)};
        for (int c = 0; c < 3; ++c) {
            const double q = (double)m[c] * cell;
            pos[3 * i + c] = wrap_pos((q + d1 * (double)psi1[c * n3 + i]) + d2 * (double)psi2[c * n3 + i], L);
            if (pres) pres[c * n3 + i] = T(0);
        }
    }
}

// CIC readout of the force at each particle (fb_paint's weights) fused with the kick and, DRIFT, the drift:
//   p_res += (F cK - dP1 Psi1) - dP2 Psi2;   x = wrap(x + (p_res Dr + dD1 Psi1) + dD2 Psi2)
// Lanes take consecutive particles, whose Lagrangian nodes are consecutive along z: the 8 x 3 gathers of a wave stay in a few
// rows of each force component.
struct KickCoef { double cK, dP1, dP2, Dr, dD1, dD2; };
template <typename T, bool DRIFT>
__global__ __launch_bounds__(256) void k_cola_kick(const T* __restrict__ F, const T* __restrict__ psi1, const T* __restrict__ psi2,
                                                   T* __restrict__ pres, double* __restrict__ pos, unsigned long long n3, int N,
                                                   double s, double L, KickCoef k) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256) {
        double x[3], w[3][2];
        unsigned long long m[3][2];
        for (int c = 0; c < 3; ++c) {
            x[c] = pos[3 * i + c];
            const double u = x[c] * s, f0 = floor(u), f = u - f0;
            m[c][0] = (unsigned long long)wrap_node((long long)f0, N);
            m[c][1] = (unsigned long long)wrap_node((long long)f0 + 1, N);
            w[c][0] = 1.0 - f; w[c][1] = f;
        }
        double g[3] = {0.0, 0.0, 0.0};
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const unsigned long long r = (m[0][a] * N + m[1][b]) * N;
                const double wab = w[0][a] * w[1][b];
                for (int e = 0; e < 2; ++e) {
                    const double wt = wab * w[2][e];
                    const unsigned long long node = r + m[2][e];
                    for (int c = 0; c < 3; ++c) g[c] += wt * (double)F[c * n3 + node];
                }
            }
        for (int c = 0; c < 3; ++c) {
            const double p1 = psi1[c * n3 + i], p2 = psi2[c * n3 + i];
            const T pn = (T)((double)pres[c * n3 + i] + ((g[c] * k.cK - k.dP1 * p1) - k.dP2 * p2));
            pres[c * n3 + i] = pn;
            if (DRIFT) pos[3 * i + c] = wrap_pos(x[c] + (((double)pn * k.Dr + k.dD1 * p1) + k.dD2 * p2), L);
        }
    }
}

// out[i stride] = fac ((p_res + P1 Psi1) + P2 Psi2), component c
template <typename T>
__global__ __launch_bounds__(256) void k_cola_velocity(const T* __restrict__ psi1, const T* __restrict__ psi2,
                                                       const T* __restrict__ pres, unsigned long long n3, double P1, double P2,
                                                       double fac, double* __restrict__ out, int stride) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256)
        out[i * stride] = fac * (((double)pres[i] + P1 * (double)psi1[i]) + P2 * (double)psi2[i]);
}

// delta = count - 1
template <typename T>
__global__ __launch_bounds__(256) void k_cola_delta(const T* __restrict__ count, T* __restrict__ delta, unsigned long long n3) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256)
        delta[i] = (T)((double)count[i] - 1.0);
}

// v = paint(w = v) / paint(w = 1), 0 where nothing was painted
template <typename T>
__global__ __launch_bounds__(256) void k_cola_vgrid(T* __restrict__ num, const T* __restrict__ count, unsigned long long n3) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (unsigned long long)gridDim.x * 256) {
        const double c = count[i];
        num[i] = c != 0.0 ? (T)((double)num[i] / c) : T(0);
    }
}

unsigned long long n3_of(const fb_plan* p) { return (unsigned long long)p->N * p->N * p->N; }

template <typename T>
int r2c(fb_plan* p, const void* in, void* half, hipStream_t s) {
    return sizeof(T) == 4 ? fbi_fft_r2c_f32(p, in, half, 0, s) : fbi_fft_r2c_f64(p, in, half, 0, s);
}
template <typename T>
int c2r(fb_plan* p, void* half, void* out, hipStream_t s) {
    const double sc = 1.0 / (double)n3_of(p);
    return sizeof(T) == 4 ? fbi_fft_c2r_f32(p, half, out, sc, s) : fbi_fft_c2r_f64(p, half, out, sc, s);
}
// out_real = c2r(mult(a, b, c) * half_in), half_work destroyed
template <typename T>
int kfield(fb_plan* p, const void* half_in, void* half_work, int a, int b, double c, void* out_real, hipStream_t s) {
    const unsigned long long n = (unsigned long long)p->N * p->NR * p->NZP;
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_cola_kmul<T>), dim3(grid_for(n, p)), dim3(256), 0, s, (const T*)half_in, (T*)half_work, p->N, p->NR,
                       p->NZP, p->L[0], a, b, c); }
    FB_LAUNCH_CHECK("k_cola_kmul");
    return c2r<T>(p, half_work, out_real, s);
}

template <typename T>
int lpt(fb_plan* p, const void* delta0, T* psi1, T* psi2, T* work3, void* h1, void* h2, hipStream_t s) {
    const unsigned long long n3 = n3_of(p);
    int r = r2c<T>(p, delta0, h1, s);
    for (int c = 0; c < 3 && !r; ++c) r = kfield<T>(p, h1, h2, c, -1, 1.0, psi1 + c * n3, s);
    // the six second derivatives: xx, yy, zz into psi2, xy, xz, yz into work3; S over work3[0]
    static const int ab[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
    T* six[6] = {psi2, psi2 + n3, psi2 + 2 * n3, work3, work3 + n3, work3 + 2 * n3};
    for (int q = 0; q < 6 && !r; ++q) r = kfield<T>(p, h1, h2, ab[q][0], ab[q][1], 1.0, six[q], s);
    if (r) return r;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cola_source<T>), dim3(grid_for(n3, p)), dim3(256), 0, s, (const T*)psi2, work3, n3); }
    FB_LAUNCH_CHECK("k_cola_source");
    r = r2c<T>(p, work3, h1, s);
    for (int c = 0; c < 3 && !r; ++c) r = kfield<T>(p, h1, h2, c, -1, -1.0, psi2 + c * n3, s);
    return r;
}

template <typename T>
int init(fb_plan* p, const T* psi1, const T* psi2, double d1, double d2, double* pos, T* pres, hipStream_t s) {
    const unsigned long long n3 = n3_of(p);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cola_init<T>), dim3(grid_for(n3, p)), dim3(256), 0, s, psi1, psi2, n3, p->N, p->L[0] / (double)p->N,
                       p->L[0], d1, d2, pos, pres); }
    FB_LAUNCH_CHECK("k_cola_init");
    return FB_OK;
}

template <typename T>
int force(fb_plan* p, const double* pos, T* count, T* delta, T* F, double coef, void* h1, void* h2, hipStream_t s) {
    const unsigned long long n3 = n3_of(p);
    int r = fb_paint(p, pos, nullptr, (int64_t)n3, FB_WINDOW_CIC, count, s);
    if (r) return r;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cola_delta<T>), dim3(grid_for(n3, p)), dim3(256), 0, s, (const T*)count, delta, n3); }
    FB_LAUNCH_CHECK("k_cola_delta");
    if (!F) return FB_OK;
    r = r2c<T>(p, delta, h1, s);
    for (int c = 0; c < 3 && !r; ++c) r = kfield<T>(p, h1, h2, c, -1, coef, F + c * n3, s);
    return r;
}

template <typename T>
int kick(fb_plan* p, const T* F, const T* psi1, const T* psi2, T* pres, double* pos, const double* cf, int drift, hipStream_t s) {
    const unsigned long long n3 = n3_of(p);
    const KickCoef k{cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]};
    const double sc = (double)p->N / p->L[0];
    { FbProfScope _ps(p, FBK_REALOP, s);
    if (drift)
        hipLaunchKernelGGL((k_cola_kick<T, true>), dim3(grid_for(n3, p)), dim3(256), 0, s, F, psi1, psi2, pres, pos, n3, p->N, sc,
                           p->L[0], k);
    else
        hipLaunchKernelGGL((k_cola_kick<T, false>), dim3(grid_for(n3, p)), dim3(256), 0, s, F, psi1, psi2, pres, pos, n3, p->N, sc,
                           p->L[0], k); }
    FB_LAUNCH_CHECK("k_cola_kick");
    return FB_OK;
}

template <typename T>
int velocity(fb_plan* p, const T* psi1, const T* psi2, const T* pres, int comp, double P1, double P2, double fac, double* out,
             int stride, hipStream_t s) {
    const unsigned long long n3 = n3_of(p), o = (unsigned long long)comp * n3;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cola_velocity<T>), dim3(grid_for(n3, p)), dim3(256), 0, s, psi1 + o, psi2 + o, pres + o, n3, P1, P2, fac,
                       out, stride); }
    FB_LAUNCH_CHECK("k_cola_velocity");
    return FB_OK;
}

template <typename T>
int grid_velocity(fb_plan* p, T* num, const T* count, hipStream_t s) {
    const unsigned long long n3 = n3_of(p);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_cola_vgrid<T>), dim3(grid_for(n3, p)), dim3(256), 0, s, num, count, n3); }
    FB_LAUNCH_CHECK("k_cola_vgrid");
    return FB_OK;
}

template <typename T>
int run(fb_plan* p, const void* delta0, int n_steps, const double* cf, double* pos, T* psi1, T* psi2, T* pres, T* F, T* count,
        T* delta, void* h1, void* h2, hipStream_t s) {
    int r = lpt<T>(p, delta0, psi1, psi2, F, h1, h2, s);
    if (!r) r = init<T>(p, psi1, psi2, cf[0], cf[1], pos, pres, s);
    if (!r && n_steps == 0) r = force<T>(p, pos, count, delta, nullptr, cf[2], h1, h2, s);
    for (int j = 0; j <= n_steps && n_steps > 0 && !r; ++j) {
        r = force<T>(p, pos, count, delta, F, cf[2], h1, h2, s);
        if (!r) r = kick<T>(p, F, psi1, psi2, pres, pos, cf + 3 + 6 * j, j < n_steps, s);
    }
    return r;
}

int cubic_check(const fb_plan* p) {
    FB_REQUIRE(p->L[0] == p->L[1] && p->L[1] == p->L[2], "COLA needs a cubic box (Lx == Ly == Lz)");
    FB_REQUIRE(!p->comm, "COLA runs on a single-GPU plan");
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_cola_lpt(fb_plan* p, const void* delta0, void* psi1, void* psi2, void* work3, void* work_half1, void* work_half2,
                void* stream) {
    FB_REQUIRE(p && delta0 && psi1 && psi2 && work3 && work_half1 && work_half2, "null pointer");
    int r = cubic_check(p);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, lpt<float>(p, delta0, (float*)psi1, (float*)psi2, (float*)work3, work_half1, work_half2, s),
                       lpt<double>(p, delta0, (double*)psi1, (double*)psi2, (double*)work3, work_half1, work_half2, s));
}

int fb_cola_init(fb_plan* p, const void* psi1, const void* psi2, double d1, double d2, double* pos, void* pres, void* stream) {
    FB_REQUIRE(p && psi1 && psi2 && pos, "null pointer");
    int r = cubic_check(p);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, init<float>(p, (const float*)psi1, (const float*)psi2, d1, d2, pos, (float*)pres, s),
                       init<double>(p, (const double*)psi1, (const double*)psi2, d1, d2, pos, (double*)pres, s));
}

int fb_cola_force(fb_plan* p, const double* pos, void* count, void* delta, void* force_out, double coef, void* work_half1,
                  void* work_half2, void* stream) {
    FB_REQUIRE(p && pos && count && delta, "null pointer");
    FB_REQUIRE(!force_out || (work_half1 && work_half2), "null pointer");
    int r = cubic_check(p);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, force<float>(p, pos, (float*)count, (float*)delta, (float*)force_out, coef, work_half1, work_half2, s),
                       force<double>(p, pos, (double*)count, (double*)delta, (double*)force_out, coef, work_half1, work_half2, s));
}

int fb_cola_kick(fb_plan* p, const void* force, const void* psi1, const void* psi2, void* pres, double* pos, const double* coef,
                 int drift, void* stream) {
    FB_REQUIRE(p && force && psi1 && psi2 && pres && pos && coef, "null pointer");
    int r = cubic_check(p);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, kick<float>(p, (const float*)force, (const float*)psi1, (const float*)psi2, (float*)pres, pos, coef, drift, s),
                       kick<double>(p, (const double*)force, (const double*)psi1, (const double*)psi2, (double*)pres, pos, coef,
                                    drift, s));
}

int fb_cola_velocity(fb_plan* p, const void* psi1, const void* psi2, const void* pres, int component, double P1, double P2,
                     double fac, double* out, int stride, void* stream) {
    FB_REQUIRE(p && psi1 && psi2 && pres && out, "null pointer");
    FB_REQUIRE(component >= 0 && component <= 2 && stride >= 1, "component must be 0, 1 or 2 and stride >= 1");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, velocity<float>(p, (const float*)psi1, (const float*)psi2, (const float*)pres, component, P1, P2, fac, out,
                                          stride, s),
                       velocity<double>(p, (const double*)psi1, (const double*)psi2, (const double*)pres, component, P1, P2, fac,
                                        out, stride, s));
}

int fb_cola_grid_velocity(fb_plan* p, void* num_inout, const void* count, void* stream) {
    FB_REQUIRE(p && num_inout && count, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, grid_velocity<float>(p, (float*)num_inout, (const float*)count, s),
                       grid_velocity<double>(p, (double*)num_inout, (const double*)count, s));
}

int fb_cola_run(fb_plan* p, const void* delta0, int n_steps, const double* coef, double* pos, void* psi1, void* psi2, void* pres,
                void* force, void* count, void* delta, void* work_half1, void* work_half2, void* stream) {
    FB_REQUIRE(p && delta0 && coef && pos && psi1 && psi2 && pres && force && count && delta && work_half1 && work_half2,
               "null pointer");
    FB_REQUIRE(n_steps >= 0, "n_steps must be >= 0");
    int r = cubic_check(p);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, run<float>(p, delta0, n_steps, coef, pos, (float*)psi1, (float*)psi2, (float*)pres, (float*)force,
                                     (float*)count, (float*)delta, work_half1, work_half2, s),
                       run<double>(p, delta0, n_steps, coef, pos, (double*)psi1, (double*)psi2, (double*)pres, (double*)force,
                                   (double*)count, (double*)delta, work_half1, work_half2, s));
}

}  // extern "C"
