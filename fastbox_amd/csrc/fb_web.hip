// Cosmic-web classification (fastbox_amd/web.py; defined by this project -- the T-web of Hahn et al. 2007 and Forero-Romero et
// al. 2009, the V-web of Hoffman et al. 2012 -- in DESIGN.md section 4 and stated in numpy in tests/web_numpy.py): the six
// component spectra of the tidal tensor of a density and of the shear tensor of a velocity, each in one pass over its input
// (the plan's c2r follows, six times), and the per-voxel eigenvalues lambda_1 >= lambda_2 >= lambda_3 of the six real component
// cubes with the void / sheet / filament / knot classes, their counts and weight sums for up to 16 thresholds.  Both plan
// precisions are compiled here; see include/fastbox_hip.h for the entry points.
//
// The multipliers and the eigen-solve are fp64 on both plans; spectra and cubes are read and written in the plan's precision.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include "fb_fft.h"                       // cx
#include "fb_kshell.h"                   // FB_TWO_PI
#include <cmath>
#include <vector>

#define FB_WEB_ROWS 4                    // (k_x, k_y) rows per workgroup of the two k-space kernels: 64 lanes each
#define FB_WEB_EIGEN_WG 8                // workgroups per compute unit of k_web_eigen: full occupancy of its lightest instantiation
#define FB_WEB_SWEEPS 6                  // cyclic Jacobi sweeps of k_web_eigen: fixed (see eigen3)

namespace {
using namespace fb;

template <typename T> struct Half6 { cx<T>* c[6]; };         // xx, yy, zz, xy, xz, yz
template <typename T> struct Half3 { const cx<T>* c[3]; };
template <typename T> struct Real6 { const T* c[6]; };
template <typename T> struct Real3 { T* c[3]; };

// Layout of a half spectrum and the box sides.  The modes are the exact signed FFT indices and k_a = (2 pi m_a) / L_a, as in
// fb_recon.hip: the plan's KGeom tables carry the reference's mode numbering, which at grids that are no power of two leaves
// some indices with mode 0 (hostgeom.mode_numbers) -- right for the reference's own fields, not for a tensor this project defines.
struct WebGeom { int N, NZV, NZP, NR; double L[3]; };
WebGeom web_geom(const fb_plan* p) { return WebGeom{p->N, p->NZV, p->NZP, p->NR, {p->L[0], p->L[1], p->L[2]}}; }
// every stored row of a half spectrum, the spare one of each x-plane included
dim3 web_rows(const fb_plan* p) { return dim3((unsigned)(((long long)p->N * p->NR + FB_WEB_ROWS - 1) / FB_WEB_ROWS)); }
__device__ __forceinline__ double web_k(int idx, int N, double L) { return (FB_TWO_PI * mode_of(idx, N)) / L; }

// T_ij(k) = k_i k_j / k^2 exp(-k^2 R^2 / 2) delta(k): delta(k) is read once, six half spectra are written.  Zero at k = 0; for
// i != j zero where m_i = -N/2 or m_j = -N/2 (index N/2); the diagonal keeps its Nyquist planes.  One (k_x, k_y) row per 64
// lanes, as k_potential; k^2 = (k_x^2 + k_y^2) + k_z^2 in fp64 on both plans.  The padding of the half layout (columns past
// N/2, the spare row of each x-plane) is not read and is written as zero: the generic c2r reads it.  A lane reads its own mode
// before it writes it and no other lane's: the outputs must not overlap each other, and the entry point keeps them off the
// input too.
template <typename T>
__global__ __launch_bounds__(64 * FB_WEB_ROWS) void k_tidal_k(const cx<T>* __restrict__ dk, Half6<T> out, WebGeom g, double RR) {
    const long long row = (long long)blockIdx.x * FB_WEB_ROWS + threadIdx.y;
    if (row >= (long long)g.N * g.NR) return;
    const int N = g.N, i = (int)(row / g.NR), j = (int)(row % g.NR), h = N >> 1;
    const long long base = row * g.NZP;
    if (j == N) {                                   // the spare row
        for (int l = threadIdx.x; l < g.NZP; l += 64)
#pragma unroll
            for (int c = 0; c < 6; ++c) out.c[c][base + l] = cx<T>{T(0), T(0)};
        return;
    }
    const double ki = web_k(i, N, g.L[0]), kj = web_k(j, N, g.L[1]);
    const double rowsum = ki * ki + kj * kj;
    const bool nyq_row = i == h || j == h;
    for (int l = threadIdx.x; l < g.NZP; l += 64) {
        double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (l >= g.NZV) {                           // the padding of the row
#pragma unroll
            for (int c = 0; c < 6; ++c) out.c[c][base + l] = cx<T>{T(0), T(0)};
            continue;
        }
        if (i | j | l) {
            const double kl = web_k(l, N, g.L[2]), k2 = rowsum + kl * kl;
            const double w = exp(-0.5 * (k2 * RR)) / k2;
            const bool nl = l == h;
            m[0] = ki * ki * w; m[1] = kj * kj * w; m[2] = kl * kl * w;
            m[3] = nyq_row ? 0.0 : ki * kj * w;
            m[4] = (i == h || nl) ? 0.0 : ki * kl * w;
            m[5] = (j == h || nl) ? 0.0 : kj * kl * w;
        }
        const cx<T> d = dk[base + l];
        const double re = (double)d.x, im = (double)d.y;
#pragma unroll
        for (int c = 0; c < 6; ++c) out.c[c][base + l] = cx<T>{(T)(m[c] * re), (T)(m[c] * im)};
    }
}

// Sigma_ij(k) = -(i / 2 H0) (k_i v_j(k) + k_j v_i(k)) exp(-k^2 R^2 / 2), the term k_i v_j zero where m_i = -N/2: the three
// velocity spectra are read once, six half spectra are written.  -i (a + i b) = b - i a.
template <typename T>
__global__ __launch_bounds__(64 * FB_WEB_ROWS) void k_shear_k(Half3<T> v, Half6<T> out, WebGeom g, double RR, double inv2H0) {
    const long long row = (long long)blockIdx.x * FB_WEB_ROWS + threadIdx.y;
    if (row >= (long long)g.N * g.NR) return;
    const int N = g.N, i = (int)(row / g.NR), j = (int)(row % g.NR), h = N >> 1;
    const long long base = row * g.NZP;
    if (j == N) {                                   // the spare row
        for (int l = threadIdx.x; l < g.NZP; l += 64)
#pragma unroll
            for (int c = 0; c < 6; ++c) out.c[c][base + l] = cx<T>{T(0), T(0)};
        return;
    }
    const double ki = web_k(i, N, g.L[0]), kj = web_k(j, N, g.L[1]);
    const double rowsum = ki * ki + kj * kj;
    for (int l = threadIdx.x; l < g.NZP; l += 64) {
        if (l >= g.NZV) {                           // the padding of the row
#pragma unroll
            for (int c = 0; c < 6; ++c) out.c[c][base + l] = cx<T>{T(0), T(0)};
            continue;
        }
        const double kl = web_k(l, N, g.L[2]), k2 = rowsum + kl * kl;
        const double w = exp(-0.5 * (k2 * RR)) * inv2H0;
        const double k[3] = {i == h ? 0.0 : ki * w, j == h ? 0.0 : kj * w, l == h ? 0.0 : kl * w};
        double re[3], im[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { const cx<T> d = v.c[a][base + l]; re[a] = (double)d.x; im[a] = (double)d.y; }
        const int I[6] = {0, 1, 2, 0, 0, 1}, J[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double sr = k[I[c]] * re[J[c]] + k[J[c]] * re[I[c]], si = k[I[c]] * im[J[c]] + k[J[c]] * im[I[c]];
            out.c[c][base + l] = cx<T>{(T)si, (T)(-sr)};
        }
    }
}

// One rotation of the cyclic sweep: annihilates a_pq; r is the third index.  a_pp and a_qq move by t a_pq (the trace is kept to
// rounding), the row r by the rotation itself.
__device__ __forceinline__ void rotate3(double& app, double& aqq, double& apq, double& arp, double& arq) {
    double c, s;
    const double t = jacobi_rotation(app, aqq, apq, c, s);
    const double hh = t * apq;
    app -= hh; aqq += hh; apq = 0.0;
    const double p = arp, q = arq;
    arp = c * p - s * q;
    arq = s * p + c * q;
}
// Eigenvalues of the symmetric 3 x 3 matrix (xx, yy, zz, xy, xz, yz), descending.  Cyclic Jacobi in registers over the pairs
// (x, y), (x, z), (y, z): every step is an orthogonal similarity, so the result is backward stable whatever the spectrum (equal
// eigenvalues included, where the closed trigonometric form loses half the digits).  FB_WEB_SWEEPS sweeps, always: the
// off-diagonal norm falls below 1e-20 of the matrix norm in four sweeps on every class of matrix tried
// and converges quadratically from there; nothing here loops on the data, so a NaN cannot keep a wave.
__device__ __forceinline__ void eigen3(const double (&a)[6], double (&lam)[3]) {
    double xx = a[0], yy = a[1], zz = a[2], xy = a[3], xz = a[4], yz = a[5];
#pragma unroll 1
    for (int sweep = 0; sweep < FB_WEB_SWEEPS; ++sweep) {
        rotate3(xx, yy, xy, xz, yz);             // (x, y): row z = (xz, yz)
        rotate3(xx, zz, xz, xy, yz);             // (x, z): row y = (xy, yz)
        rotate3(yy, zz, yz, xy, xz);             // (y, z): row x = (xy, xz)
    }
    double t;
    if (xx < yy) { t = xx; xx = yy; yy = t; }
    if (yy < zz) { t = yy; yy = zz; zz = t; }
    if (xx < yy) { t = xx; xx = yy; yy = t; }
    lam[0] = xx; lam[1] = yy; lam[2] = zz;
}

// sum of an unsigned over the 64 lanes, in every lane
__device__ __forceinline__ unsigned wave_count(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// NT thresholds' worth of per-lane accumulators (nt <= NT; the thresholds beyond nt are +inf and their rows are not read):
// counts and fp64 weight sums [NT][4] in registers, with compile-time indices only.  At the end the workgroup's counts go
// through LDS integer atomics to 64-bit device totals (integers: no order), the weight sums through a fixed tree (wave
// shuffles, then the four waves in order) to partial[value][workgroup], which k_bin_finish<> sums in workgroup order.
// The grid is FB_WEB_EIGEN_WG workgroups per compute unit at most, each walking its voxels: the 16-threshold instantiation
// runs one workgroup per compute unit at a time, and the prologue and the reductions above are paid once per workgroup.
template <typename T, int NT>
__global__ __launch_bounds__(256) void k_web_eigen(Real6<T> comp, unsigned long long nv, const double* __restrict__ thr, int nt,
                                                   int class_at, const T* __restrict__ weight, Real3<T> eig,
                                                   unsigned char* __restrict__ classes, unsigned long long* __restrict__ counts,
                                                   double* __restrict__ wpartial, unsigned long long* __restrict__ n_nan) {
    __shared__ unsigned long long cnt_s[NT * 4 + 1];
    double t[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) t[j] = j < nt ? thr[j] : INFINITY;
    unsigned cnt[NT][4];
    double ws[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) { cnt[j][c] = 0u; ws[j][c] = 0.0; }
    unsigned bad = 0u;
    for (int q = threadIdx.x; q < NT * 4 + 1; q += 256) cnt_s[q] = 0ull;

    // (a wave's 32-bit counts hold its own voxels: 2^33 / (4 x 8 x compute units) of them at 2048^3)
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (unsigned long long)gridDim.x * 256) {
        double a[6], lam[3];
        bool finite = true;
#pragma unroll
        for (int c = 0; c < 6; ++c) { a[c] = (double)comp.c[c][v]; finite = finite && fabs(a[c]) <= 1.7976931348623157e308; }
        int cls_out = 255;
        if (finite) {                                // (components near the largest double can still overflow in the solve)
            eigen3(a, lam);
            finite = fabs(lam[0]) <= 1.7976931348623157e308 && fabs(lam[1]) <= 1.7976931348623157e308 &&
                     fabs(lam[2]) <= 1.7976931348623157e308;
        }
        if (finite) {
            const double w = weight ? (double)weight[v] : 0.0;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int cls = (lam[0] > t[j] ? 1 : 0) + (lam[1] > t[j] ? 1 : 0) + (lam[2] > t[j] ? 1 : 0);
                if (j == class_at) cls_out = cls;
#pragma unroll
                for (int c = 0; c < 4; ++c) { cnt[j][c] += cls == c ? 1u : 0u; ws[j][c] += cls == c ? w : 0.0; }
            }
        } else {
            lam[0] = lam[1] = lam[2] = __builtin_nan("");
            ++bad;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (eig.c[c]) eig.c[c][v] = (T)lam[c];
        if (classes) classes[v] = (unsigned char)cls_out;
    }

    __syncthreads();
    // each wave sums its lanes' counts (below 2^32: a workgroup of the capped grid holds fewer voxels), one LDS add per wave
    const bool lane0 = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned n = wave_count(cnt[j][c]);
            if (lane0 && n) atomicAdd(&cnt_s[j * 4 + c], (unsigned long long)n);
        }
    bad = wave_count(bad);
    if (lane0 && bad) atomicAdd(&cnt_s[NT * 4], (unsigned long long)bad);
    if (wpartial) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double s = block_reduce(ws[j][c], 0);
                if (threadIdx.x == 0 && j < nt) wpartial[(size_t)(j * 4 + c) * gridDim.x + blockIdx.x] = s;
            }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nt * 4; q += 256)
        if (cnt_s[q]) atomicAdd(&counts[q], cnt_s[q]);
    if (threadIdx.x == 0 && cnt_s[NT * 4]) atomicAdd(n_nan, cnt_s[NT * 4]);
}

// out = 1 where classes == kind, else 0
template <typename T>
__global__ __launch_bounds__(256) void k_web_mask(const unsigned char* __restrict__ classes, unsigned long long nv, int kind,
                                                  T* __restrict__ out) {
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (unsigned long long)gridDim.x * 256)
        out[v] = classes[v] == kind ? T(1) : T(0);
}
template <typename T>
int mask(fb_plan* p, const uint8_t* classes, int kind, void* out, hipStream_t s) {
    const unsigned long long nv = (unsigned long long)p->N * p->N * p->N;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_web_mask<T>), dim3(grid_for(nv, p)), dim3(256), 0, s, classes, nv, kind, (T*)out); }
    FB_LAUNCH_CHECK("k_web_mask");
    return FB_OK;
}

template <typename T>
int tidal(fb_plan* p, const void* half_in, void* const* out6, double R, hipStream_t s) {
    Half6<T> o;
    for (int c = 0; c < 6; ++c) o.c[c] = (cx<T>*)out6[c];
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_tidal_k<T>), web_rows(p), dim3(64, FB_WEB_ROWS), 0, s, (const cx<T>*)half_in, o, web_geom(p), R * R); }
    FB_LAUNCH_CHECK("k_tidal_k");
    return FB_OK;
}

template <typename T>
int shear(fb_plan* p, const void* const* vel3, void* const* out6, double R, double H0, hipStream_t s) {
    Half3<T> v;
    Half6<T> o;
    for (int c = 0; c < 3; ++c) v.c[c] = (const cx<T>*)vel3[c];
    for (int c = 0; c < 6; ++c) o.c[c] = (cx<T>*)out6[c];
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_shear_k<T>), web_rows(p), dim3(64, FB_WEB_ROWS), 0, s, v, o, web_geom(p), R * R, 0.5 / H0); }
    FB_LAUNCH_CHECK("k_shear_k");
    return FB_OK;
}

template <typename T>
int eigen(fb_plan* p, const void* const* comp6, const double* thr_host, int nt, int class_at, const void* weight, void* const* eig3,
          uint8_t* classes, uint64_t* counts_out, double* wsum_out, uint64_t* n_nan_out, hipStream_t s) {
    const unsigned long long nv = (unsigned long long)p->N * p->N * p->N;
    const unsigned long long blocks = (nv + 255) / 256, cap = (unsigned long long)FB_WEB_EIGEN_WG * p->num_cu;
    const int grid = (int)(blocks < cap ? blocks : cap), nq = nt * 4;
    const bool sums = wsum_out && weight;
    // work: thresholds [16], counts [64] and n_nan [1], the weight sums [64], their partials [64][grid]
    const size_t head = FB_WEB_NT_MAX + FB_WEB_NT_MAX * 4 + 1 + FB_WEB_NT_MAX * 4;
    FB_TRY(p->work.ensure((head + (sums ? (size_t)nq * grid : 0)) * 8));
    double* thr_dev = p->work.as<double>();
    unsigned long long* cnt_dev = reinterpret_cast<unsigned long long*>(thr_dev + FB_WEB_NT_MAX);
    unsigned long long* nan_dev = cnt_dev + FB_WEB_NT_MAX * 4;
    double* wsum_dev = reinterpret_cast<double*>(nan_dev + 1);
    double* wpart_dev = sums ? wsum_dev + FB_WEB_NT_MAX * 4 : nullptr;
    if (nt) FB_HIP(hipMemcpyAsync(thr_dev, thr_host, (size_t)nt * 8, hipMemcpyHostToDevice, s));
    FB_HIP(hipMemsetAsync(cnt_dev, 0, (FB_WEB_NT_MAX * 4 + 1) * 8, s));
    Real6<T> a;
    Real3<T> e;
    for (int c = 0; c < 6; ++c) a.c[c] = (const T*)comp6[c];
    for (int c = 0; c < 3; ++c) e.c[c] = eig3 ? (T*)eig3[c] : nullptr;
    const T* w = sums ? (const T*)weight : nullptr;
    {
        FbProfScope _ps(p, FBK_REALOP, s);
        if (nt <= 1)
            hipLaunchKernelGGL((k_web_eigen<T, 1>), dim3(grid), dim3(256), 0, s, a, nv, thr_dev, nt, class_at, w, e, classes, cnt_dev,
                               wpart_dev, nan_dev);
        else if (nt <= 4)
            hipLaunchKernelGGL((k_web_eigen<T, 4>), dim3(grid), dim3(256), 0, s, a, nv, thr_dev, nt, class_at, w, e, classes, cnt_dev,
                               wpart_dev, nan_dev);
        else
            hipLaunchKernelGGL((k_web_eigen<T, FB_WEB_NT_MAX>), dim3(grid), dim3(256), 0, s, a, nv, thr_dev, nt, class_at, w, e, classes,
                               cnt_dev, wpart_dev, nan_dev);
    }
    FB_LAUNCH_CHECK("k_web_eigen");
    if (sums && nq) {
        FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL(k_bin_finish<>, dim3(nq), dim3(256), 0, s, wpart_dev, grid, nq, wsum_dev);
        FB_LAUNCH_CHECK("k_bin_finish");
    }
    if (!(counts_out || wsum_out || n_nan_out)) return FB_OK;
    std::vector<unsigned long long> h(FB_WEB_NT_MAX * 4 + 1 + FB_WEB_NT_MAX * 4);
    FB_TRY(fb_read_back(h.data(), cnt_dev, h.size() * 8, s));
    if (counts_out) for (int q = 0; q < nq; ++q) counts_out[q] = h[q];
    if (n_nan_out) *n_nan_out = h[FB_WEB_NT_MAX * 4];
    if (wsum_out) {
        const double* ws = reinterpret_cast<const double*>(h.data() + FB_WEB_NT_MAX * 4 + 1);
        for (int q = 0; q < nq; ++q) wsum_out[q] = sums ? ws[q] : 0.0;
    }
    return FB_OK;
}

bool distinct(const void* const* a, int n, const void* const* b, int nb) {
    for (int i = 0; i < n; ++i) {
        if (!a[i]) return false;
        for (int j = i + 1; j < n; ++j) if (a[i] == a[j]) return false;
        for (int j = 0; j < nb; ++j) if (a[i] == b[j]) return false;
    }
    return true;
}

}  // namespace

extern "C" {

int fb_tidal_k(fb_plan* p, const void* half_in, void* const* half_out6, double R, void* stream) {
    FB_REQUIRE(p && half_in && half_out6, "null pointer");
    FB_REQUIRE(distinct(half_out6, 6, &half_in, 1), "six distinct output spectra, none of them the input");
    FB_REQUIRE(R >= 0.0 && R < 1e150, "smoothing must be >= 0 and finite");
    FB_REQUIRE(!p->comm, "the cosmic-web kernels run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, tidal<float>(p, half_in, half_out6, R, s), tidal<double>(p, half_in, half_out6, R, s));
}

int fb_shear_k(fb_plan* p, const void* const* half_vel3, void* const* half_out6, double R, double H0, void* stream) {
    FB_REQUIRE(p && half_vel3 && half_out6, "null pointer");
    FB_REQUIRE(half_vel3[0] && half_vel3[1] && half_vel3[2], "null pointer");
    FB_REQUIRE(distinct(half_out6, 6, half_vel3, 3), "six distinct output spectra, none of them an input");
    FB_REQUIRE(R >= 0.0 && R < 1e150, "smoothing must be >= 0 and finite");
    FB_REQUIRE(H0 > 0.0 && H0 < 1e300, "H0 must be positive and finite");
    FB_REQUIRE(!p->comm, "the cosmic-web kernels run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, shear<float>(p, half_vel3, half_out6, R, H0, s), shear<double>(p, half_vel3, half_out6, R, H0, s));
}

int fb_web_eigen(fb_plan* p, const void* const* comp6, const double* thresholds, int nt, int class_at, const void* weight,
                 void* const* eig3, uint8_t* classes, uint64_t* counts_out, double* wsum_out, uint64_t* n_nan_out, void* stream) {
    FB_REQUIRE(p && comp6, "null pointer");
    for (int c = 0; c < 6; ++c) FB_REQUIRE(comp6[c], "null pointer");
    FB_REQUIRE(nt >= 0 && nt <= FB_WEB_NT_MAX, "nt must be between 0 and 16");
    FB_REQUIRE(nt == 0 || thresholds, "null pointer");
    FB_REQUIRE(nt > 0 || !(classes || counts_out || wsum_out), "classes, counts and weight sums need a threshold");
    FB_REQUIRE(!classes || (class_at >= 0 && class_at < nt), "class_at must be a threshold index");
    bool finite = true, ascending = true;
    for (int j = 0; j < nt; ++j) {
        finite = finite && std::fabs(thresholds[j]) <= 1.7976931348623157e308;
        ascending = ascending && (j == 0 || thresholds[j] > thresholds[j - 1]);
    }
    FB_REQUIRE(finite, "thresholds must be finite");
    FB_REQUIRE(ascending, "thresholds must be strictly ascending");
    FB_REQUIRE(!p->comm, "the cosmic-web kernels run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    if (!classes) class_at = -1;
    return FB_DISPATCH(p, eigen<float>(p, comp6, thresholds, nt, class_at, weight, eig3, classes, counts_out, wsum_out, n_nan_out, s),
                       eigen<double>(p, comp6, thresholds, nt, class_at, weight, eig3, classes, counts_out, wsum_out, n_nan_out, s));
}

int fb_web_mask(fb_plan* p, const uint8_t* classes, int kind, void* real_out, void* stream) {
    FB_REQUIRE(p && classes && real_out, "null pointer");
    FB_REQUIRE(kind >= 0 && kind <= 3, "kind must be 0 (void), 1 (sheet), 2 (filament) or 3 (knot)");
    FB_REQUIRE(!p->comm, "the cosmic-web kernels run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, mask<float>(p, classes, kind, real_out, s), mask<double>(p, classes, kind, real_out, s));
}

}  // extern "C"
