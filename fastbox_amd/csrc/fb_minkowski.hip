// Minkowski functionals of excursion sets (fastbox_amd/minkowski.py; defined by this project -- Schmalzing & Buchert 1997, the
// Crofton estimates on the lattice -- in DESIGN.md section 4 and stated in numpy in tests/minkowski_numpy.py): the counts of
// cells, faces, edges and vertices of the cell complex of {field >= t} for up to 256 thresholds in one pass over the cube, for
// the periodic box (3-D) or for every frequency channel as a periodic 2-D map, and the per-channel moments about given means.
// Both plan precisions are compiled here; see include/fastbox_hip.h for the entry points.
//
// An element of the complex lies in the set at t iff the maximum of its adjacent voxels is >= t.  bin(v) = #{j : t_j <= v} is
// monotone in v, so an element's bin is the integer maximum of its voxels' bins: one binary search per voxel (fp64 compare on
// the stored value), the bins of a tile and its +1 halo as 16-bit words in LDS, then 8 (3-D) or 4 (per channel) integer maxima
// per voxel, each adding 1 to a 32-bit LDS histogram over the nt + 1 threshold intervals.  Workgroups walk the tiles and add
// their histograms to 64-bit device totals at the end (integer atomics: the totals do not depend on the order).  The host
// forms the cumulative sums from above.  Work memory: the thresholds and the histograms (the plan's shared work buffer).
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <cmath>
#include <vector>

#define FB_MK_MAX_NT 256
#define FB_MK_TX3 8                       // the 3-D tile: 8 x 8 x 32 own voxels, 9 x 9 x 33 read (1.31 reads per voxel)
#define FB_MK_TY3 8
#define FB_MK_TZ3 32
#define FB_MK_MOMENT_BLOCKS 512          // pixel slices of fb_channel_moments (fb_channel_means' count)

namespace {
using namespace fb;

// Tile of one workgroup pass: TX x TY x TZ own voxels and their +x, +y (3-D: +z) neighbours.  3-D: the LDS histogram is kept in
// C interleaved copies (copy = lane mod C, copies of one counter in adjacent banks): a Gaussian field puts most of a wave's
// updates into a few intervals, and C copies divide the same-address serialisation of those by C.  Per channel the lanes of a
// wave lie in TZ different channels (z is the fastest axis), each with a histogram of its own at an odd word stride.
struct MkGeom {
    int TX, TY, TZ, C;
    int thr_rows;            // threshold rows held in LDS: 1, or TZ (mode 2: a row per channel)
    int hstride;             // per channel: words per channel of the LDS histogram (odd)
    size_t lds;              // dynamic LDS bytes
};

// #{j : t_j <= d} for ascending t; 0 for a NaN, nt for +inf
__device__ __forceinline__ int bin_of(const double* __restrict__ t, int nt, double d) {
    int lo = 0, hi = nt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= d) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// D3: hist[8][nt + 1] in the order n3, n2x, n2y, n2z, n1x, n1y, n1z, n0; grid (workgroups, 1), each walking the tiles of the box.
// !D3: hist[N][4][nt + 1] in the order n2, n1x, n1y, n0; grid (workgroups, z chunks), each walking the (x, y) tiles of its chunk.
// thr: [nt] or (row_stride = nt) [N][nt].  n_nan: one word, or [N].
template <typename T, bool D3>
__global__ __launch_bounds__(256) void k_minkowski(const T* __restrict__ f, int N, const double* __restrict__ thr, int nt,
                                                   int row_stride, MkGeom g, unsigned long long* __restrict__ hist,
                                                   unsigned long long* __restrict__ n_nan) {
    extern __shared__ double mk_lds[];
    // (the 3-D tile is a compile-time constant, so that its index arithmetic is shifts and multiplies)
    const int TX = D3 ? FB_MK_TX3 : g.TX, TY = D3 ? FB_MK_TY3 : g.TY, TZ = D3 ? FB_MK_TZ3 : g.TZ, nb = nt + 1;
    const int EZ = TZ + (D3 ? 1 : 0), EY = TY + 1, EX = TX + 1;
    const int nhist = D3 ? 8 * nb * g.C : TZ * g.hstride, nnan = D3 ? 1 : TZ;
    double* thr_s = mk_lds;
    unsigned* hist_s = reinterpret_cast<unsigned*>(thr_s + g.thr_rows * nt);
    unsigned* nan_s = hist_s + nhist;
    unsigned short* bins = reinterpret_cast<unsigned short*>(nan_s + nnan);
    const int tid = threadIdx.x;
    const int zc0 = D3 ? 0 : (int)blockIdx.y * TZ;         // per channel: this workgroup's first channel

    for (int i = tid; i < g.thr_rows * nt; i += 256) {
        const int r = i / nt, j = i - r * nt, c = zc0 + r;
        thr_s[i] = (row_stride == 0 || c < N) ? thr[(size_t)(row_stride ? c : 0) * row_stride + j] : 0.0;
    }
    for (int i = tid; i < nhist + nnan; i += 256) hist_s[i] = 0u;      // nan_s follows hist_s
    __syncthreads();

    const int ntx = (N + TX - 1) / TX, nty = (N + TY - 1) / TY, ntz = D3 ? (N + TZ - 1) / TZ : 1;
    const long long ntiles = (long long)ntx * nty * ntz;
    const int sy = EZ, sx = EY * EZ, nload = EX * sx, nown = TX * TY * TZ;
    const int copy = tid & (g.C - 1);

    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tz = (int)(t % ntz), ty = (int)((t / ntz) % nty), tx = (int)(t / ((long long)ntz * nty));
        const int x0 = tx * TX, y0 = ty * TY, z0 = D3 ? tz * TZ : zc0;
        // the tile's bins; a voxel past the box's far face is the periodic image at 0; one further out is never read
        for (int i = tid; i < nload; i += 256) {
            const int lz = i % EZ, ly = (i / EZ) % EY, lx = i / sx;
            int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            int b = 0;
            if (gx <= N && gy <= N && (D3 ? gz <= N : gz < N)) {
                const bool own = lx < TX && ly < TY && lz < TZ && gx < N && gy < N && gz < N;
                gx = gx == N ? 0 : gx; gy = gy == N ? 0 : gy; gz = gz == N ? 0 : gz;
                const double d = (double)f[((size_t)gx * N + gy) * N + gz];
                b = bin_of(thr_s + (g.thr_rows > 1 ? lz * nt : 0), nt, d);
                if (own && d != d) atomicAdd(&nan_s[D3 ? 0 : lz], 1u);
            }
            bins[i] = (unsigned short)b;
        }
        __syncthreads();
        for (int i = tid; i < nown; i += 256) {
            const int lz = i % TZ, ly = (i / TZ) % TY, lx = i / (TZ * TY);
            if (x0 + lx >= N || y0 + ly >= N || z0 + lz >= N) continue;
            const unsigned short* q = bins + lx * sx + ly * sy + lz;
            const int a = q[0], ax = q[sx], ay = q[sy], axy = q[sx + sy];
            if (D3) {
                const int az = q[1], axz = q[sx + 1], ayz = q[sy + 1], axyz = q[sx + sy + 1];
                const int fx = imax(a, ax), fy = imax(a, ay), fz = imax(a, az);
                const int e[8] = {a, fx, fy, fz, imax(fy, imax(az, ayz)), imax(fx, imax(az, axz)), imax(fx, imax(ay, axy)),
                                  imax(imax(fx, imax(ay, axy)), imax(imax(az, axz), imax(ayz, axyz)))};
#pragma unroll
                for (int k = 0; k < 8; ++k) atomicAdd(&hist_s[(k * nb + e[k]) * g.C + copy], 1u);
            } else {
                // edge d runs along d: its two pixels differ in the other axis
                const int e[4] = {a, imax(a, ay), imax(a, ax), imax(imax(a, ax), imax(ay, axy))};
                unsigned* h = hist_s + lz * g.hstride;
#pragma unroll
                for (int k = 0; k < 4; ++k) atomicAdd(&h[k * nb + e[k]], 1u);
            }
        }
        __syncthreads();
    }

    if (D3) {
        for (int i = tid; i < 8 * nb; i += 256) {
            unsigned long long s = 0;
            for (int c = 0; c < g.C; ++c) s += hist_s[i * g.C + c];
            if (s) atomicAdd(&hist[i], s);
        }
        if (tid == 0 && nan_s[0]) atomicAdd(n_nan, (unsigned long long)nan_s[0]);
    } else {
        for (int i = tid; i < TZ * 4 * nb; i += 256) {
            const int lz = i / (4 * nb), r = i - lz * 4 * nb;
            const unsigned v = hist_s[lz * g.hstride + r];
            if (zc0 + lz < N && v) atomicAdd(&hist[(size_t)(zc0 + lz) * 4 * nb + r], (unsigned long long)v);
        }
        for (int lz = tid; lz < TZ; lz += 256)
            if (zc0 + lz < N && nan_s[lz]) atomicAdd(&n_nan[zc0 + lz], (unsigned long long)nan_s[lz]);
    }
}

// partial[block][2][channel] = sum over the block's pixels of (v - m_c) and (v - m_c)^2, fp64, four chains in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void k_channel_moment_sums(const T* __restrict__ cube, const double* __restrict__ mean,
                                                             double* __restrict__ partial, long long npix, int N) {
#pragma clang fp contract(off)
    const long long per = (npix + gridDim.x - 1) / gridDim.x;
    const long long p0 = (long long)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    for (int c = threadIdx.x; c < N; c += blockDim.x) {
        const double m = mean[c];
        double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
        long long p = p0;
        for (; p + 3 < p1; p += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double d = (double)cube[(p + u) * N + c] - m;
                a[u] += d; b[u] += d * d;
            }
        }
        for (; p < p1; ++p) {
            const double d = (double)cube[p * N + c] - m;
            a[0] += d; b[0] += d * d;
        }
        partial[((size_t)blockIdx.x * 2) * N + c] = (a[0] + a[1]) + (a[2] + a[3]);
        partial[((size_t)blockIdx.x * 2 + 1) * N + c] = (b[0] + b[1]) + (b[2] + b[3]);
    }
}
// out[q][c] = sum over the blocks, in block order
__global__ __launch_bounds__(256) void k_channel_moment_finish(const double* __restrict__ partial, int nblocks, int N,
                                                               double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * N) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)b * 2 * N + i];
    out[i] = s;
}

MkGeom geometry(int nt, int mode) {
    MkGeom g;
    const int nb = nt + 1;
    if (mode == 0) {
        g.TX = FB_MK_TX3; g.TY = FB_MK_TY3; g.TZ = FB_MK_TZ3;
        g.C = nb <= 64 ? 16 : nb <= 128 ? 8 : 4;               // 8 nb C words: at most 33 KiB
        g.thr_rows = 1; g.hstride = 0;
        g.lds = (size_t)nt * 8 + (size_t)(8 * nb * g.C + 1) * 4 + (size_t)(g.TX + 1) * (g.TY + 1) * (g.TZ + 1) * 2;
    } else {
        // 4096 own voxels a tile; as many channels as keep TZ (4 nb + 1) words near 32 KiB and (mode 2) TZ nt thresholds in 16 KiB
        g.TZ = nb <= 32 ? 64 : nb <= 64 ? 32 : nb <= 128 ? 16 : 8;
        g.TX = g.TZ >= 32 ? 8 : 16;
        g.TY = 4096 / (g.TX * g.TZ);
        g.C = 1;
        g.thr_rows = mode == 2 ? g.TZ : 1;
        g.hstride = 4 * nb + 1;
        g.lds = (size_t)g.thr_rows * nt * 8 + (size_t)(g.TZ * g.hstride + g.TZ) * 4 + (size_t)(g.TX + 1) * (g.TY + 1) * g.TZ * 2;
    }
    return g;
}

template <typename T>
int counts(fb_plan* p, const void* real, const double* thr_host, int nt, int mode, uint64_t* counts_out, uint64_t* n_nan_out,
           hipStream_t s) {
    const int N = p->N, nb = nt + 1;
    const size_t rows = mode == 2 ? N : 1, nthr = rows * nt;
    const size_t nhist = mode == 0 ? (size_t)8 * nb : (size_t)N * 4 * nb, nnan = mode == 0 ? 1 : N;
    FB_TRY(p->work.ensure((nthr + nhist + nnan) * 8));
    double* thr_dev = p->work.as<double>();
    unsigned long long* hist_dev = reinterpret_cast<unsigned long long*>(thr_dev + nthr);
    unsigned long long* nan_dev = hist_dev + nhist;
    FB_HIP(hipMemcpyAsync(thr_dev, thr_host, nthr * 8, hipMemcpyHostToDevice, s));
    FB_HIP(hipMemsetAsync(hist_dev, 0, (nhist + nnan) * 8, s));
    const MkGeom g = geometry(nt, mode);
    const long long ntx = (N + g.TX - 1) / g.TX, nty = (N + g.TY - 1) / g.TY, ntz = (N + g.TZ - 1) / g.TZ;
    {
        FbProfScope _ps(p, FBK_REALOP, s);
        if (mode == 0) {
            // a workgroup's 32-bit counters hold its own voxels only: at least one workgroup per 2^31 voxels (2048^3 is 2^33)
            const long long ntiles = ntx * nty * ntz, vox = (long long)N * N * N;
            long long wg = 4ll * p->num_cu > (vox >> 31) + 1 ? 4ll * p->num_cu : (vox >> 31) + 1;
            if (wg > ntiles) wg = ntiles;
            hipLaunchKernelGGL((k_minkowski<T, true>), dim3((unsigned)wg), dim3(256), g.lds, s, (const T*)real, N, thr_dev, nt, 0, g,
                               hist_dev, nan_dev);
        } else {
            long long wg = 4ll * p->num_cu / ntz;              // a channel has N^2 <= 2^22 pixels
            if (wg < 1) wg = 1;
            if (wg > ntx * nty) wg = ntx * nty;
            hipLaunchKernelGGL((k_minkowski<T, false>), dim3((unsigned)wg, (unsigned)ntz), dim3(256), g.lds, s, (const T*)real, N,
                               thr_dev, nt, mode == 2 ? nt : 0, g, hist_dev, nan_dev);
        }
    }
    FB_LAUNCH_CHECK("k_minkowski");
    std::vector<unsigned long long> h(nhist + nnan);
    FB_TRY(fb_read_back(h.data(), hist_dev, h.size() * 8, s));
    // counts[j] = the elements with bin > j: the cumulative sum from above
    if (mode == 0) {
        for (int e = 0; e < 8; ++e) {
            unsigned long long acc = 0;
            for (int j = nt - 1; j >= 0; --j) { acc += h[(size_t)e * nb + j + 1]; counts_out[(size_t)e * nt + j] = acc; }
        }
    } else {
        for (int c = 0; c < N; ++c)
            for (int e = 0; e < 4; ++e) {
                unsigned long long acc = 0;
                for (int j = nt - 1; j >= 0; --j) {
                    acc += h[((size_t)c * 4 + e) * nb + j + 1];
                    counts_out[((size_t)e * N + c) * nt + j] = acc;
                }
            }
    }
    for (size_t i = 0; i < nnan; ++i) n_nan_out[i] = h[nhist + i];
    return FB_OK;
}

template <typename T>
int moments(fb_plan* p, const void* cube, const double* mean_dev, double* out_dev, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    const int nb = FB_MK_MOMENT_BLOCKS < npix ? FB_MK_MOMENT_BLOCKS : (int)npix;
    FB_TRY(p->work.ensure((size_t)nb * 2 * N * sizeof(double)));
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_channel_moment_sums<T>), dim3(nb), dim3(256), 0, s, (const T*)cube, mean_dev, p->work.as<double>(), npix, N);
    hipLaunchKernelGGL(k_channel_moment_finish, dim3((2 * N + 255) / 256), dim3(256), 0, s, p->work.as<const double>(), nb, N, out_dev);
    FB_LAUNCH_CHECK("k_channel_moments");
    return FB_OK;
}

}  // namespace

extern "C" {

int fb_minkowski_counts(fb_plan* p, const void* real, const double* thresholds, int nt, int mode, uint64_t* counts_out,
                        uint64_t* n_nan_out, void* stream) {
    FB_REQUIRE(p && real && thresholds && counts_out && n_nan_out, "null pointer");
    FB_REQUIRE(nt >= 1 && nt <= FB_MK_MAX_NT, "nt must be between 1 and 256");
    FB_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (3-D), 1 (per channel) or 2 (per channel, a threshold row each)");
    FB_REQUIRE(!p->comm, "Minkowski functionals run on a single-GPU plan");
    const size_t rows = mode == 2 ? p->N : 1;
    bool finite = true, ascending = true;
    for (size_t r = 0; r < rows; ++r)
        for (int j = 0; j < nt; ++j) {
            const double t = thresholds[r * nt + j];
            finite = finite && std::fabs(t) <= 1.7976931348623157e308;
            ascending = ascending && (j == 0 || t > thresholds[r * nt + j - 1]);
        }
    FB_REQUIRE(finite, "thresholds must be finite");
    FB_REQUIRE(ascending, "thresholds must be strictly ascending");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, counts<float>(p, real, thresholds, nt, mode, counts_out, n_nan_out, s),
                       counts<double>(p, real, thresholds, nt, mode, counts_out, n_nan_out, s));
}

int fb_channel_moments(fb_plan* p, const void* cube, const double* mean_dev, double* out_dev, void* stream) {
    FB_REQUIRE(p && cube && mean_dev && out_dev, "null pointer");
    FB_REQUIRE(!p->comm, "Minkowski functionals run on a single-GPU plan");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, moments<float>(p, cube, mean_dev, out_dev, s), moments<double>(p, cube, mean_dev, out_dev, s));
}

}  // extern "C"
