// Putting data onto a grid (the reference's fastbox/analysis.py:31-118): trilinear regridding of a cube given on rectilinear
// coordinates, and the histogram of a catalogue.  Both plan precisions are compiled here; see include/fastbox_hip.h for the
// definitions and DESIGN.md section 4 for the design.
//
// No contraction anywhere in this file: cell membership and the interpolation weights are compared with numpy statements
// (tests/regrid_numpy.py) that round every product and sum.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <algorithm>
#include <cmath>

#define FB_REGRID_SMALL (1 << 16)        // bytes of halo_small, as fb_halo.hip sizes it
#define FB_REGRID_RED_BLOCKS 2048        // workgroups of the sum |w| reduction (fb_paint's)
#define FB_REGRID_RANGE_BLOCKS 512       // workgroups of the position range: 9 rows of partials fit halo_small
#define FB_REGRID_CHUNKS 256             // row chunks of the channel means
#define FB_REGRID_SEARCH_STEPS 32        // halvings of a binary search over fewer than 2^31 nodes

namespace {
using namespace fb;

// the number of g[i] <= p among g[0..n): np.searchsorted(g, p, 'right') for an ascending g; a bounded loop
__device__ __forceinline__ int upper_bound(const double* __restrict__ g, int n, double p) {
    int lo = 0, hi = n;
    for (int it = 0; it < FB_REGRID_SEARCH_STEPS && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (g[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- regridding -------------------------------------------------------------------------------------------------------------
// Per axis a (blockIdx.y) and new coordinate p: the cell i = clip(searchsorted(g, p, 'right') - 1, 0, n - 2) and the fraction
// t = (p - g[i]) / (g[i + 1] - g[i]); cell -1 and t = NaN where p lies outside [g[0], g[n - 1]] or is NaN.
struct LocAxes {
    const double* g[3];
    const double* p[3];
    int ng[3], np[3];
    int* cell[3];
    double* frac[3];
};
__global__ __launch_bounds__(256) void k_regrid_locate(LocAxes A) {
    const int a = blockIdx.y;
    const double* __restrict__ g = a == 0 ? A.g[0] : a == 1 ? A.g[1] : A.g[2];
    const double* __restrict__ pp = a == 0 ? A.p[0] : a == 1 ? A.p[1] : A.p[2];
    int* __restrict__ cell = a == 0 ? A.cell[0] : a == 1 ? A.cell[1] : A.cell[2];
    double* __restrict__ frac = a == 0 ? A.frac[0] : a == 1 ? A.frac[1] : A.frac[2];
    const int n = a == 0 ? A.ng[0] : a == 1 ? A.ng[1] : A.ng[2];
    const int np = a == 0 ? A.np[0] : a == 1 ? A.np[1] : A.np[2];
    const double first = g[0], last = g[n - 1];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < np; j += gridDim.x * 256) {
        const double p = pp[j];
        int c = -1;
        double t = NAN;
        if (p >= first && p <= last) {
            c = upper_bound(g, n, p) - 1;
            c = c < 0 ? 0 : (c > n - 2 ? n - 2 : c);
            t = (p - g[c]) / (g[c + 1] - g[c]);
        }
        cell[j] = c;
        frac[j] = t;
    }
}

// Channel means of a [nrow][nz] cube over the voxels that are not NaN, in fp64 and a fixed order: workgroup (z block, chunk)
// sums rows chunk * rpc + {ty, ty + 4, ...} of 64 channels, consecutive lanes on consecutive channels, then the four row
// lanes as (0 + 1) + (2 + 3); the finish adds chunks ty, ty + 4, ... per row lane, joins the four the same way and divides:
// 0 / 0 = NaN for an all-NaN channel.
template <typename T>
__global__ __launch_bounds__(256) void k_regrid_chan_partial(const T* __restrict__ cube, long long nrow, int nz, long long rpc,
                                                             double* __restrict__ psum, double* __restrict__ pcnt) {
    __shared__ double sh[2][4][64];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int z = blockIdx.x * 64 + tx;
    const long long r0 = (long long)blockIdx.y * rpc;
    const long long r1 = r0 + rpc < nrow ? r0 + rpc : nrow;
    double s = 0.0, c = 0.0;
    if (z < nz)
        for (long long r = r0 + ty; r < r1; r += 4) {
            const double v = (double)cube[(unsigned long long)r * nz + z];
            if (v == v) { s += v; c += 1.0; }
        }
    sh[0][ty][tx] = s;
    sh[1][ty][tx] = c;
    __syncthreads();
    if (ty == 0 && z < nz) {
        psum[(size_t)blockIdx.y * nz + z] = (sh[0][0][tx] + sh[0][1][tx]) + (sh[0][2][tx] + sh[0][3][tx]);
        pcnt[(size_t)blockIdx.y * nz + z] = (sh[1][0][tx] + sh[1][1][tx]) + (sh[1][2][tx] + sh[1][3][tx]);
    }
}
__global__ __launch_bounds__(256) void k_regrid_chan_finish(const double* __restrict__ psum, const double* __restrict__ pcnt,
                                                            int nchunk, int nz, double* __restrict__ mean) {
    __shared__ double sh[2][4][64];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int z = blockIdx.x * 64 + tx;
    double s = 0.0, c = 0.0;
    if (z < nz)
        for (int q = ty; q < nchunk; q += 4) { s += psum[(size_t)q * nz + z]; c += pcnt[(size_t)q * nz + z]; }
    sh[0][ty][tx] = s;
    sh[1][ty][tx] = c;
    __syncthreads();
    if (ty == 0 && z < nz)
        mean[z] = ((sh[0][0][tx] + sh[0][1][tx]) + (sh[0][2][tx] + sh[0][3][tx])) /
                  ((sh[1][0][tx] + sh[1][1][tx]) + (sh[1][2][tx] + sh[1][3][tx]));
}

// One lane per z_new and FB_REGRID_ROWS output rows per thread: a workgroup is 64 consecutive z_new by 4 FB_REGRID_ROWS rows, thread
// (tx, ty) taking rows ty, ty + 4, ...  The x and y cells are uniform over a row of lanes, the z tables and the store are
// coalesced, the eight corner loads of neighbouring lanes fall on the same or the next input element, and the z cell, its
// fraction and the two channel means are loaded once for all rows of a thread.  All corner loads of a thread are issued before
// the first is used (a point outside reads cell 0 and is overwritten): with one voxel per thread the kernel waited on two
// dependent round trips per wave and ran at a quarter of this speed.  A NaN corner reads as its channel's mean.
// The sum is scipy's: value = 0, then for every corner (x outermost, z innermost) value += v * ((wx * wy) * wz) -- zero weights
// included, so a NaN corner of weight 0 gives NaN.  out is [n0][n1][npz] with (n0, n1) = (npy, npx) when swap_xy (numpy's 'xy'
// meshgrid) and (npx, npy) otherwise; 64-bit indexing.
#define FB_REGRID_ROWS 4
template <typename T>
__global__ __launch_bounds__(256) void k_regrid(const T* __restrict__ cube, int ny, int nz, const double* __restrict__ mean,
                                                const int* __restrict__ cx, const int* __restrict__ cy, const int* __restrict__ cz,
                                                const double* __restrict__ fx, const double* __restrict__ fy,
                                                const double* __restrict__ fz, long long nrows, int n1, int npz, int swap_xy,
                                                int nzb, T* __restrict__ out) {
    constexpr int R = FB_REGRID_ROWS;
    const unsigned b = blockIdx.x;
    const long long row0 = (long long)(b / (unsigned)nzb) * (4 * R) + threadIdx.y;
    const int k = (int)(b % (unsigned)nzb) * 64 + threadIdx.x;
    if (k >= npz) return;
    const int ck = cz[k];
    const int ckc = ck < 0 ? 0 : ck;
    const double tz = fz[k];
    const double wz[2] = {1.0 - tz, tz};
    const double m[2] = {mean[ckc], mean[ckc + 1]};
    const bool narrow = nrows <= 0x7fffffffll;                    // the usual case: a 32-bit division per row
    bool outside[R];
    double wxy[R][4];
    const T* src[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long row = row0 + 4 * r < nrows ? row0 + 4 * r : nrows - 1;
        const long long oa = narrow ? (long long)((unsigned)row / (unsigned)n1) : row / n1;
        const long long ob = row - oa * n1;
        const long long ix = swap_xy ? ob : oa, iy = swap_xy ? oa : ob;
        const int ci = cx[ix], cj = cy[iy];
        outside[r] = (ci | cj | ck) < 0;
        const double tx = fx[ix], ty = fy[iy];
        wxy[r][0] = (1.0 - tx) * (1.0 - ty); wxy[r][1] = (1.0 - tx) * ty;
        wxy[r][2] = tx * (1.0 - ty);         wxy[r][3] = tx * ty;
        src[r] = cube + ((unsigned long long)(ci < 0 ? 0 : ci) * ny + (cj < 0 ? 0 : cj)) * nz + ckc;
    }
    T v[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q) v[r][q] = src[r][((unsigned long long)(q >> 2) * ny + ((q >> 1) & 1)) * nz + (q & 1)];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row0 + 4 * r >= nrows) break;
        double value = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double u = v[r][q] == v[r][q] ? (double)v[r][q] : m[q & 1];
            value += u * (wxy[r][q >> 1] * wz[q & 1]);
        }
        out[(unsigned long long)(row0 + 4 * r) * npz + k] = outside[r] ? (T)NAN : (T)value;
    }
}

template <typename T>
int regrid(fb_plan* p, const void* cube, int nx, int ny, int nz, const double* gx, const double* gy, const double* gz,
           const double* px, int npx, const double* py, int npy, const double* pz, int npz, int swap_xy, void* out, hipStream_t s) {
    const long long nrow = (long long)nx * ny;
    const int nchunk = (int)std::min<long long>(FB_REGRID_CHUNKS, (nrow + 63) / 64);
    const long long rpc = (nrow + nchunk - 1) / nchunk;
    const size_t npt = (size_t)npx + npy + npz;
    const long long n0 = swap_xy ? npy : npx;
    const int n1 = swap_xy ? npx : npy;
    const long long nrows = n0 * n1;
    const int nzb = (npz + 63) / 64;
    const long long nblocks = (nrows + 4 * FB_REGRID_ROWS - 1) / (4 * FB_REGRID_ROWS) * nzb;
    FB_REQUIRE(nblocks < (1ll << 31), "fb_regrid_trilinear: the output takes 2^31 workgroups or more");
    // work: frac [npt] | mean [nz] | psum [nchunk][nz] | pcnt [nchunk][nz] | cell [npt] int
    const size_t nd = npt + (size_t)nz * (1 + 2 * (size_t)nchunk);
    FB_TRY(p->work.ensure(nd * sizeof(double) + npt * sizeof(int)));
    double* frac = p->work.as<double>();
    double* mean = frac + npt;
    double* psum = mean + nz;
    double* pcnt = psum + (size_t)nchunk * nz;
    int* cell = (int*)(pcnt + (size_t)nchunk * nz);
    LocAxes A;
    A.g[0] = gx; A.g[1] = gy; A.g[2] = gz;
    A.p[0] = px; A.p[1] = py; A.p[2] = pz;
    A.ng[0] = nx; A.ng[1] = ny; A.ng[2] = nz;
    A.np[0] = npx; A.np[1] = npy; A.np[2] = npz;
    A.cell[0] = cell; A.cell[1] = cell + npx; A.cell[2] = cell + npx + npy;
    A.frac[0] = frac; A.frac[1] = frac + npx; A.frac[2] = frac + npx + npy;
    const int npmax = std::max(npx, std::max(npy, npz));
    hipLaunchKernelGGL(k_regrid_locate, dim3(std::min((npmax + 255) / 256, 1024), 3), dim3(256), 0, s, A);
    FB_LAUNCH_CHECK("k_regrid_locate");
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_regrid_chan_partial<T>), dim3((nz + 63) / 64, nchunk), dim3(64, 4), 0, s, (const T*)cube, nrow, nz, rpc,
                       psum, pcnt); }
    FB_LAUNCH_CHECK("k_regrid_chan_partial");
    hipLaunchKernelGGL(k_regrid_chan_finish, dim3((nz + 63) / 64), dim3(64, 4), 0, s, (const double*)psum, (const double*)pcnt,
                       nchunk, nz, mean);
    FB_LAUNCH_CHECK("k_regrid_chan_finish");
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_regrid<T>), dim3((unsigned)nblocks), dim3(64, 4), 0, s, (const T*)cube, ny, nz, (const double*)mean,
                       (const int*)A.cell[0], (const int*)A.cell[1], (const int*)A.cell[2], (const double*)A.frac[0],
                       (const double*)A.frac[1], (const double*)A.frac[2], nrows, n1, npz, swap_xy, nzb, (T*)out); }
    FB_LAUNCH_CHECK("k_regrid");
    return FB_OK;
}

// ---- catalogue histogram ------------------------------------------------------------------------------------------------------
// The bin of p among the edges e[0..n]: np.histogramdd's searchsorted(e, p, 'right') - 1 with p == e[n] in bin n - 1, and -1
// for p outside [e[0], e[n]] or NaN.  From the arithmetic guess (p - e[0]) n / (e[n] - e[0]) two steps against the table;
// whatever they leave undecided goes to the bounded binary search.  The table decides: the same doubles numpy compares with.
__device__ __forceinline__ int hist_bin(const double* __restrict__ e, int n, double p, double scale) {
    if (!(p >= e[0] && p <= e[n])) return -1;
    const double g = (p - e[0]) * scale;
    int j = g < (double)(n - 1) ? (int)g : n - 1;
    j = j < 0 ? 0 : j;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (j > 0 && p < e[j]) --j;
        else if (j < n - 1 && p >= e[j + 1]) ++j;
    }
    if (!(e[j] <= p && (j == n - 1 || p < e[j + 1]))) {
        j = upper_bound(e, n + 1, p) - 1;
        j = j > n - 1 ? n - 1 : j;
    }
    return j;
}
// fb_paint's fixed point (fb_dev.h) on the histogram's cells: one add of round(w 2^F) per particle that falls inside
template <bool TWO>
__global__ __launch_bounds__(256) void k_grid_catalogue(const double* __restrict__ pos, const double* __restrict__ wt,
                                                        unsigned long long n, const double* __restrict__ ex, int nx,
                                                        const double* __restrict__ ey, int ny, const double* __restrict__ ez, int nz,
                                                        const double* __restrict__ wsum, unsigned long long* acc_hi,
                                                        unsigned long long* acc_lo) {
    const int F = fx_exponent(wsum[0], 61) + (TWO ? 32 : 0);
    const double scale = ldexp(1.0, F);
    const double sx = (double)nx / (ex[nx] - ex[0]), sy = (double)ny / (ey[ny] - ey[0]), sz = (double)nz / (ez[nz] - ez[0]);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int bx = hist_bin(ex, nx, pos[3 * i], sx);
        const int by = hist_bin(ey, ny, pos[3 * i + 1], sy);
        const int bz = hist_bin(ez, nz, pos[3 * i + 2], sz);
        if ((bx | by | bz) < 0) continue;
        const double v = (wt ? wt[i] : 1.0) * scale;
        const unsigned long long c = ((unsigned long long)bx * ny + by) * nz + bz;
        if (TWO) {
            unsigned long long hi, lo;
            fx_split(v, hi, lo);
            atomicAdd(&acc_hi[c], hi);
            atomicAdd(&acc_lo[c], lo);
        } else {
            atomicAdd(&acc_hi[c], (unsigned long long)__double2ll_rn(v));
        }
    }
}

template <typename T>
int grid_catalogue(fb_plan* p, const double* pos, const double* wt, unsigned long long n, const double* ex, int nx,
                   const double* ey, int ny, const double* ez, int nz, void* out, hipStream_t s) {
    const unsigned long long nv = (unsigned long long)nx * ny * nz;
    constexpr bool TWO = sizeof(T) == 8;
    FB_TRY(p->halo_small.ensure(FB_REGRID_SMALL));
    FB_TRY(p->halo_acc.ensure(nv * 8 * (TWO ? 2 : 1)));
    double* part = p->halo_small.as<double>();
    double* wsum = part + FB_REGRID_RED_BLOCKS;
    unsigned long long* hi = p->halo_acc.as<unsigned long long>();
    unsigned long long* lo = TWO ? hi + nv : nullptr;
    FB_HIP(hipMemsetAsync(hi, 0, nv * 8 * (TWO ? 2 : 1), s));
    const int nb = std::min(grid_for(n, p), FB_REGRID_RED_BLOCKS);
    hipLaunchKernelGGL(k_paint_wsum<>, dim3(nb), dim3(256), 0, s, wt, n, part);
    FB_LAUNCH_CHECK("k_paint_wsum");
    hipLaunchKernelGGL(k_halo_finish<>, dim3(1), dim3(256), 0, s, (const double*)part, nb, 0, wsum);
    FB_LAUNCH_CHECK("k_halo_finish");
    if (n) {
        FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL((k_grid_catalogue<TWO>), dim3(grid_for(n, p)), dim3(256), 0, s, pos, wt, n, ex, nx, ey, ny, ez, nz,
                           (const double*)wsum, hi, lo);
    }
    FB_LAUNCH_CHECK("k_grid_catalogue");
    hipLaunchKernelGGL((k_paint_finish<T, TWO>), dim3(grid_for(nv, p)), dim3(256), 0, s, (const unsigned long long*)hi,
                       (const unsigned long long*)lo, nv, (const double*)wsum, (T*)out);
    FB_LAUNCH_CHECK("k_paint_finish");
    return FB_OK;
}

// ---- position range -----------------------------------------------------------------------------------------------------------
// partials[q][workgroup], q = 0..5: -min x, max x, -min y, max y, -min z, max z over the values that are not NaN (fmax: a NaN
// loses); q = 6, 7, 8: 1 where a NaN was seen on x, y, z.  The finish takes the maximum of each row.
__global__ __launch_bounds__(256) void k_position_range(const double* __restrict__ pos, unsigned long long n, int nb,
                                                        double* __restrict__ partials) {
    double r[9] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = pos[3 * i + a];
            if (x != x) r[6 + a] = 1.0;
            r[2 * a] = fmax(r[2 * a], -x);
            r[2 * a + 1] = fmax(r[2 * a + 1], x);
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const double v = block_reduce(r[q], 1);
        if (threadIdx.x == 0) partials[(size_t)q * nb + blockIdx.x] = v;
    }
}
__global__ __launch_bounds__(256) void k_position_range_finish(const double* __restrict__ partials, int nb, double* __restrict__ out) {
    const double* src = partials + (size_t)blockIdx.x * nb;
    double acc = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += 256) acc = fmax(acc, src[i]);
    acc = block_reduce(acc, 1);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

}  // namespace

extern "C" {

int fb_regrid_trilinear(fb_plan* p, const void* cube, int nx, int ny, int nz, const double* gx, const double* gy, const double* gz,
                        const double* px, int npx, const double* py, int npy, const double* pz, int npz, int swap_xy, void* out,
                        void* stream) {
    FB_REQUIRE(p && cube && gx && gy && gz && px && py && pz && out, "null pointer");
    FB_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "fb_regrid_trilinear: every axis of the cube needs two nodes or more");
    FB_REQUIRE(npx >= 1 && npy >= 1 && npz >= 1, "fb_regrid_trilinear: every new axis needs one point or more");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, regrid<float>(p, cube, nx, ny, nz, gx, gy, gz, px, npx, py, npy, pz, npz, swap_xy ? 1 : 0, out, s),
                       regrid<double>(p, cube, nx, ny, nz, gx, gy, gz, px, npx, py, npy, pz, npz, swap_xy ? 1 : 0, out, s));
}

int fb_grid_catalogue(fb_plan* p, const double* pos, const double* weights, int64_t n, const double* edges_x, int nx,
                      const double* edges_y, int ny, const double* edges_z, int nz, void* out, void* stream) {
    FB_REQUIRE(p && out && edges_x && edges_y && edges_z && (pos || n == 0), "null pointer");
    FB_REQUIRE(n >= 0, "n must be >= 0");
    FB_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "fb_grid_catalogue: one cell or more along every axis");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, grid_catalogue<float>(p, pos, weights, (unsigned long long)n, edges_x, nx, edges_y, ny, edges_z, nz, out, s),
                       grid_catalogue<double>(p, pos, weights, (unsigned long long)n, edges_x, nx, edges_y, ny, edges_z, nz, out, s));
}

int fb_position_range(fb_plan* p, const double* pos, int64_t n, double* lohi6, void* stream) {
    FB_REQUIRE(p && pos && lohi6, "null pointer");
    FB_REQUIRE(n >= 1, "fb_position_range: one position or more");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    FB_TRY(p->halo_small.ensure(FB_REGRID_SMALL));
    double* part = p->halo_small.as<double>();
    double* res = part + 9 * FB_REGRID_RANGE_BLOCKS;
    const int nb = std::min(grid_for((unsigned long long)n, p), FB_REGRID_RANGE_BLOCKS);
    hipLaunchKernelGGL(k_position_range, dim3(nb), dim3(256), 0, s, pos, (unsigned long long)n, nb, part);
    FB_LAUNCH_CHECK("k_position_range");
    hipLaunchKernelGGL(k_position_range_finish, dim3(9), dim3(256), 0, s, (const double*)part, nb, res);
    FB_LAUNCH_CHECK("k_position_range_finish");
    double h[9];
    FB_TRY(fb_read_back(h, res, sizeof(h), s));
    for (int a = 0; a < 3; ++a) {
        lohi6[2 * a] = h[6 + a] != 0.0 ? NAN : -h[2 * a];
        lohi6[2 * a + 1] = h[6 + a] != 0.0 ? NAN : h[2 * a + 1];
    }
    return FB_OK;
}

}  // extern "C"
