// Interferometer sampling of a cube whose last axis is frequency: the uv-coverage counts of a set of projected baselines in
// every channel, their per-channel sums, and the per-voxel weighting of a cube transformed over its transverse axes.  The count
// rule, the weightings and the normalisers are defined in include/fastbox_hip.h and DESIGN.md section 4; the host layer is
// fastbox_amd/interferometer.py.  All three kernels put 64 consecutive channels of one transverse row in a wave, so every
// load, store and atomic add of a wave runs along the fastest axis.  Both plan precisions are compiled here.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_fft.h"                      // cx<T>
#include <algorithm>

namespace fb {
namespace {

#define FB_UV_ROWS 4                     // waves per workgroup: threadIdx.y

// ---- coverage ---------------------------------------------------------------------------------------------------------------
// A task is (sample, block of 64 channels); a wave takes tasks t = wave id, wave id + all waves, ... < ns nchunk.  The cell
// (a, b) of a baseline moves outward by |b| / (c dnu) cells over the band, so across the 64 channels of a wave it changes
// rarely: the wave's adds are a few contiguous runs along c (256 bytes when it does not change at all).  The adds are integer:
// exact and independent of the order in which they arrive.
__global__ __launch_bounds__(64 * FB_UV_ROWS) void k_uv_coverage(const double* __restrict__ samples, const int32_t* __restrict__ mult,
                                                                 long long ns, const double* __restrict__ sx,
                                                                 const double* __restrict__ sy, int32_t* __restrict__ counts,
                                                                 int N, int nchunk) {
    const long long ntask = ns * nchunk, step = (long long)gridDim.x * FB_UV_ROWS;
    const double half = (double)(N >> 1);
    for (long long t = (long long)blockIdx.x * FB_UV_ROWS + threadIdx.y; t < ntask; t += step) {
        const long long s = t / nchunk;
        const int c = (int)(t - s * nchunk) * 64 + (int)threadIdx.x;
        if (c >= N) continue;
        const double a = rint(samples[2 * s] * sx[c]), b = rint(samples[2 * s + 1] * sy[c]);
        if (!(fabs(a) <= half && fabs(b) <= half)) continue;                   // (a NaN product is rejected too)
        const int m = mult ? mult[s] : 1;
        const int ia = (int)a, ib = (int)b;
        const int i = ia < 0 ? ia + N : ia, j = ib < 0 ? ib + N : ib;          // a mod N, b mod N: -N/2 and N/2 share row N/2
        const int ic = i ? N - i : 0, jc = j ? N - j : 0;                      // -a mod N, -b mod N
        atomicAdd(&counts[((size_t)i * N + j) * N + c], m);
        atomicAdd(&counts[((size_t)ic * N + jc) * N + c], m);                  // a self-conjugate cell receives 2 m
    }
}

// ---- per-channel sums ---------------------------------------------------------------------------------------------------------
// Workgroup (x, y) owns channels [64 x, 64 x + 64) and the transverse rows 4 y + wave, + 4 gridDim.y, ...; the four waves are
// added through LDS and the workgroup adds its two int64 partials per channel to out (zeroed by the launcher).  Integer sums.
__global__ __launch_bounds__(64 * FB_UV_ROWS) void k_uv_sums(const int32_t* __restrict__ counts, unsigned long long* __restrict__ out,
                                                             int N) {
    __shared__ long long sh[2][FB_UV_ROWS][64];
    const int lane = threadIdx.x, wave = threadIdx.y, c = blockIdx.x * 64 + lane;
    const long long rows = (long long)N * N, step = (long long)gridDim.y * FB_UV_ROWS;
    long long tot = 0, cells = 0;
    if (c < N)
        for (long long r = (long long)blockIdx.y * FB_UV_ROWS + wave; r < rows; r += step) {
            const int v = counts[(size_t)r * N + c];
            tot += v;
            cells += v > 0;
        }
    sh[0][wave][lane] = tot;
    sh[1][wave][lane] = cells;
    __syncthreads();
    if (wave == 0 && c < N) {
#pragma unroll
        for (int w = 1; w < FB_UV_ROWS; ++w) { tot += sh[0][w][lane]; cells += sh[1][w][lane]; }
        atomicAdd(&out[c], (unsigned long long)tot);
        atomicAdd(&out[N + c], (unsigned long long)cells);
    }
}

// ---- weighting ------------------------------------------------------------------------------------------------------------------
// cube[row][c] *= f(S[row][c]) scale[c]: the factor in fp64, each component multiplied in fp64 and rounded once to T.
template <typename T, int MODE>
__global__ __launch_bounds__(64 * FB_UV_ROWS) void k_uv_weight(cx<T>* __restrict__ cube, const int32_t* __restrict__ counts,
                                                               const double* __restrict__ scale, int N) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= N) return;
    const double sc = scale[c];
    const long long rows = (long long)N * N, step = (long long)gridDim.y * FB_UV_ROWS;
    for (long long r = (long long)blockIdx.y * FB_UV_ROWS + threadIdx.y; r < rows; r += step) {
        const size_t at = (size_t)r * N + c;
        const int v = counts[at];
        const double f = (MODE == 0 ? (double)v : MODE == 1 ? (v > 0 ? 1.0 : 0.0) : sqrt((double)v)) * sc;
        const cx<T> z = cube[at];
        cube[at] = cx<T>{(T)((double)z.x * f), (T)((double)z.y * f)};
    }
}

inline int uv_chunks(const fb_plan* p) { return (p->N + 63) / 64; }
// row groups of a launch: all of them up to `cap` workgroups over the whole grid
inline unsigned uv_row_groups(const fb_plan* p, long long cap) {
    const long long groups = ((long long)p->N * p->N + FB_UV_ROWS - 1) / FB_UV_ROWS;
    return (unsigned)std::max(1LL, std::min({groups, cap / uv_chunks(p), 65535LL}));
}

template <typename T> int uv_weight(fb_plan* p, void* cube, const int32_t* counts, int mode, const double* scale, hipStream_t s) {
    const dim3 grid(uv_chunks(p), uv_row_groups(p, 64LL * p->num_cu)), block(64, FB_UV_ROWS);
    FbProfScope _ps(p, FBK_REALOP, s);
    if (mode == 0) hipLaunchKernelGGL((k_uv_weight<T, 0>), grid, block, 0, s, (cx<T>*)cube, counts, scale, p->N);
    else if (mode == 1) hipLaunchKernelGGL((k_uv_weight<T, 1>), grid, block, 0, s, (cx<T>*)cube, counts, scale, p->N);
    else hipLaunchKernelGGL((k_uv_weight<T, 2>), grid, block, 0, s, (cx<T>*)cube, counts, scale, p->N);
    FB_LAUNCH_CHECK("k_uv_weight");
    return FB_OK;
}

}  // namespace
}  // namespace fb

using namespace fb;

extern "C" {

int fb_uv_coverage(fb_plan* p, const double* samples_dev, const int32_t* mult_dev, int64_t ns, const double* sx_dev,
                   const double* sy_dev, int32_t* counts_dev, int accumulate, void* stream) {
    FB_REQUIRE(p && sx_dev && sy_dev && counts_dev, "null pointer");
    FB_REQUIRE(ns >= 0 && (samples_dev || ns == 0), "ns >= 0 samples");
    FB_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
    FB_REQUIRE(p->N % 2 == 0, "the uv grid needs an even N");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const size_t n3 = (size_t)p->N * p->N * p->N;
    if (!accumulate) FB_HIP(hipMemsetAsync(counts_dev, 0, n3 * sizeof(int32_t), s));
    if (ns == 0) return FB_OK;
    const int nchunk = uv_chunks(p);
    FB_REQUIRE(ns <= INT64_MAX / nchunk, "too many samples");
    const long long groups = ((long long)ns * nchunk + FB_UV_ROWS - 1) / FB_UV_ROWS;
    const unsigned grid = (unsigned)std::min(groups, 8LL * p->num_cu);          // 8 waves per SIMD, resident; they walk the tasks
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_uv_coverage, dim3(grid), dim3(64, FB_UV_ROWS), 0, s, samples_dev, mult_dev, (long long)ns, sx_dev, sy_dev,
                       counts_dev, p->N, nchunk);
    FB_LAUNCH_CHECK("k_uv_coverage");
    return FB_OK;
}

int fb_uv_channel_sums(fb_plan* p, const int32_t* counts_dev, int64_t* out_dev, void* stream) {
    FB_REQUIRE(p && counts_dev && out_dev, "null pointer");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    FB_HIP(hipMemsetAsync(out_dev, 0, 2 * (size_t)p->N * sizeof(int64_t), s));
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_uv_sums, dim3(uv_chunks(p), uv_row_groups(p, 8LL * p->num_cu)), dim3(64, FB_UV_ROWS), 0, s, counts_dev,
                       (unsigned long long*)out_dev, p->N);
    FB_LAUNCH_CHECK("k_uv_sums");
    return FB_OK;
}

int fb_uv_weight(fb_plan* p, void* full_cube_inout, const int32_t* counts_dev, int mode, const double* scale_dev, void* stream) {
    FB_REQUIRE(p && full_cube_inout && counts_dev && scale_dev, "null pointer");
    FB_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (natural), 1 (uniform) or 2 (square root)");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, uv_weight<float>(p, full_cube_inout, counts_dev, mode, scale_dev, s),
                       uv_weight<double>(p, full_cube_inout, counts_dev, mode, scale_dev, s));
}

}  // extern "C"
