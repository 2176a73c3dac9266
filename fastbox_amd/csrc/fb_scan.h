// The exclusive scan of the library: out[j] = sum of the terms j' < j for j = 0..M, so out[M] is the total.  Three launches:
// the sums of chunks of FB_SCAN_CH terms, a scan of the chunk sums in one workgroup, the chunks themselves.  The accumulated
// type A (unsigned or unsigned long long: integer adds, any order) is that of the output; term j comes from a small functor,
//   ScanPlain{in}  in[j]                       the cell histogram of fb_cells.h; the minima per tile and the root flags of fb_voids.hip
//   CatTerm{H, nb} (j / nb) H[j]               the (count, tile) table of the halo catalogue (fb_halo.hip)
// out needs M + 1 entries and csum scan_chunks(M).
#pragma once
#include "fb_plan.h"

#define FB_SCAN_PER 16                   // terms per lane
#define FB_SCAN_CH (256 * FB_SCAN_PER)   // terms per chunk = per workgroup

namespace fb {

struct ScanPlain {
    const unsigned* in;
    __device__ unsigned operator()(unsigned long long j) const { return in[j]; }
};
template <typename A, typename F>
__device__ __forceinline__ A scan_term(const F& f, unsigned long long j, unsigned long long M) { return j < M ? (A)f(j) : (A)0; }

template <typename A, typename F>
static __global__ __launch_bounds__(256) void k_exscan_chunks(F f, unsigned long long M, A* csum) {
    const unsigned long long j0 = (unsigned long long)blockIdx.x * FB_SCAN_CH;
    A s = 0;
    for (int q = 0; q < FB_SCAN_PER; ++q) s += scan_term<A>(f, j0 + (unsigned long long)q * 256 + threadIdx.x, M);
    __shared__ A tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    atomicAdd(&tot, s);
    __syncthreads();
    if (threadIdx.x == 0) csum[blockIdx.x] = tot;
}
// exclusive scan of v[0..256) in LDS (Hillis-Steele), returns this lane's prefix; `total` receives the sum
template <typename A>
static __device__ A block_exscan(A v, A* total) {
    __shared__ A sh[256];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const A a = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : (A)0;
        __syncthreads();
        sh[threadIdx.x] += a;
        __syncthreads();
    }
    const A incl = sh[threadIdx.x];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}
// one workgroup: csum[0..nc) -> exclusive prefix sums in place, 256 at a time with the running sum carried across the rounds
template <typename A>
static __global__ __launch_bounds__(256) void k_exscan_top(A* csum, int nc) {
    A carry = 0;
    for (int base = 0; base < nc; base += 256) {
        const int i = base + threadIdx.x;
        const A v = i < nc ? csum[i] : (A)0;
        A tot;
        const A ex = block_exscan(v, &tot);
        if (i < nc) csum[i] = carry + ex;
        carry += tot;
    }
}
// lane t of chunk r takes the 16 consecutive terms j0 + 16 t ..
template <typename A, typename F>
static __global__ __launch_bounds__(256) void k_exscan_apply(F f, unsigned long long M, const A* csum, A* out) {
    const unsigned long long j0 = (unsigned long long)blockIdx.x * FB_SCAN_CH + (unsigned long long)threadIdx.x * FB_SCAN_PER;
    A w[FB_SCAN_PER], s = 0;
    for (int q = 0; q < FB_SCAN_PER; ++q) { w[q] = scan_term<A>(f, j0 + q, M); s += w[q]; }
    A tot;
    A run = csum[blockIdx.x] + block_exscan(s, &tot);
    for (int q = 0; q < FB_SCAN_PER; ++q) {
        if (j0 + q <= M) out[j0 + q] = run;
        run += w[q];
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// chunks (= workgroups, = entries of csum) of a scan of M terms: the M + 1 outputs, FB_SCAN_CH to a chunk
inline unsigned long long scan_chunks(unsigned long long M) { return (M + 1 + FB_SCAN_CH - 1) / FB_SCAN_CH; }

template <typename A, typename F>
int exscan(F f, unsigned long long M, A* csum, A* out, hipStream_t s) {
    const int nc = (int)scan_chunks(M);
    hipLaunchKernelGGL((k_exscan_chunks<A, F>), dim3(nc), dim3(256), 0, s, f, M, csum);
    FB_LAUNCH_CHECK("k_exscan_chunks");
    hipLaunchKernelGGL((k_exscan_top<A>), dim3(1), dim3(256), 0, s, csum, nc);
    FB_LAUNCH_CHECK("k_exscan_top");
    hipLaunchKernelGGL((k_exscan_apply<A, F>), dim3(nc), dim3(256), 0, s, f, M, (const A*)csum, out);
    FB_LAUNCH_CHECK("k_exscan_apply");
    return FB_OK;
}

}  // namespace fb
