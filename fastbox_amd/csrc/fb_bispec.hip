// Bispectrum in triangle bins (the FFT estimator of Scoccimarro 2000 / Sefusatti et al. 2016): the stored half spectrum is split
// into k shells, every shell is transformed back with the plan's own c2r, and one sweep over the voxels contracts all triples
// of shell cubes on the fp64 matrix cores.  Both plan precisions are compiled here; see include/fastbox_hip.h for the
// definition and DESIGN.md for the algorithm, its registers and its limits.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"                      // mode_of, wave_sum, k_bin_finish
#include "fb_fft.h"                      // cx<T>
#include "fb_kshell.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define FB_BK_MAX_SHELLS 32   // two 16-row tiles of the contraction
#define FB_BK_SPLIT 4         // shells written per read of the spectrum (work_shells holds up to this many half spectra)
#define FB_BK_RUN 64          // voxels of every cube a workgroup stages at a time

namespace fb {
namespace {

struct BkSplitArgs {
    double thr[FB_BK_MAX_SHELLS + 1];   // T_b = sq_threshold(edge b): shell of k2 = #{b : T_b <= k2} - 1
    double kf[3];                       // 2 pi / L_a
    int N, NZV, NZP, NR;
    int nb, b0, nq;                     // shells b0 .. b0 + nq - 1 are written (and summed) by this launch
};

// Shell split.  One (k_x, k_y) row of the half spectrum per wave, lanes along k_z; every stored cell (padding included) of the
// nq shell spectra is written: the mode where it belongs to the shell, zero elsewhere.  UNIT: the spectrum is 1 on every mode
// (the cubes U_b that count triangles) and `half` is not read.  Along a row k2 grows with k_z, so the shells met in a 64-lane
// step are those between lane 0's and lane 63's: their sums (modes, |k|, |D|^2; cells with 0 < m_z < N/2 twice, as k_pk_bin)
// are masked wave sums in shell order.  Per-workgroup partials [value][workgroup], then k_bin_finish: no atomics.
template <typename T, bool UNIT>
__global__ __launch_bounds__(256)
void k_bk_split(const cx<T>* __restrict__ half, cx<T>* __restrict__ shells, long long shell_stride,
                double* __restrict__ partial, BkSplitArgs a) {
    __shared__ double tk[FB_BK_MAX_SHELLS + 1];
    __shared__ double acc[4][3][FB_BK_SPLIT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = a.nb, N = a.N, nq = a.nq, b0 = a.b0;
    if (tid <= nb) tk[tid] = a.thr[tid];
    if (tid < 4 * 3 * FB_BK_SPLIT) (&acc[0][0][0])[tid] = 0.0;
    __syncthreads();
    const long long nrows = (long long)N * a.NR;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < nrows; row += (long long)gridDim.x * 4) {
        const int i = (int)(row / a.NR), j = (int)(row % a.NR);
        const bool live = j < N;                                      // (row N of a plane is padding)
        const double kperp2 = live ? sq2((double)mode_of(i, N) * a.kf[0], (double)mode_of(j, N) * a.kf[1]) : 0.0;
        const long long base = row * a.NZP;
        for (int l0 = 0; l0 < a.NZP; l0 += 64) {
            const int l = l0 + lane;
            const bool in = live && l < a.NZV;
            cx<T> d{0, 0};
            if (in) d = UNIT ? cx<T>{1, 0} : half[base + l];
            const double k2 = add_sq(kperp2, (double)l * a.kf[2]);  // l <= N / 2: the stored k_z are the non-negative ones
            int key = 0x7fffffff;                                     // padding: beyond every shell
            if (in) {
                key = -1;                                             // k = 0, or below the first edge
                if (k2 > 0.0) {
                    int lo = 0, hi = nb + 1;                          // number of thresholds <= k2
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tk[mid] <= k2) lo = mid + 1; else hi = mid; }
                    key = lo - 1;                                     // nb: at or beyond the last edge
                }
            }
            if (l < a.NZP) {
                for (int q = 0; q < nq; ++q)
                    shells[(long long)q * shell_stride + base + l] = key == b0 + q ? d : cx<T>{0, 0};
            }
            const int kfirst = __shfl(key, 0, 64), klast = __shfl(key, 63, 64);
            const int lo = kfirst > b0 ? kfirst : b0, hi = klast < b0 + nq - 1 ? klast : b0 + nq - 1;
            if (lo <= hi) {
                const double w = (l == 0 || 2 * l == N) ? 1.0 : 2.0;
                const double wr = w * sqrt(k2);
                const double wp = w * ((double)d.x * (double)d.x + (double)d.y * (double)d.y);
                for (int b = lo; b <= hi; ++b) {
                    const bool mine = key == b;
                    const double s0 = wave_sum(mine ? w : 0.0), s1 = wave_sum(mine ? wr : 0.0), s2 = wave_sum(mine ? wp : 0.0);
                    if (lane == 0) { acc[wave][0][b - b0] += s0; acc[wave][1][b - b0] += s1; acc[wave][2][b - b0] += s2; }
                }
            }
        }
    }
    __syncthreads();
    if (tid < 3 * nq) {
        const int v = tid / nq, q = tid % nq;
        const double s = (acc[0][v][q] + acc[1][v][q]) + (acc[2][v][q] + acc[3][v][q]);
        partial[(size_t)tid * gridDim.x + blockIdx.x] = s;            // [value][workgroup]: see k_bin_finish
    }
}

// Triple contraction: sum_x I_b1(x) I_b2(x) I_b3(x) for every b1, b2, b3 in one sweep over the voxels.  For a fixed third
// shell it is the matrix product C[b1][b2] = sum_x (I_b1 I_b3)(x) I_b2(x), a rank-4 update per v_mfma_f64_16x16x4_f64 with the
// operand layout documented at k_channel_cov (fb_field_kernels.h): A is 16 shells b1 x 4 voxels (lane l: shell l & 15, voxel
// l >> 4), B is 4 voxels x 16 shells b2 in the same lanes, so one LDS read serves both and A only needs the product with
// I_b3 of the lane's voxel (fp64, VALU).  A workgroup of four waves stages FB_BK_RUN voxels of all cubes in LDS as fp64 (the
// next run is in flight in registers meanwhile); wave w owns the third shells b3 = w, w + 4, ..  NT = 1: nb <= 16, one tile
// per b3.  NT = 2: nb <= 32; a b3 < 16 needs the tile (b1 < 16, b2 < 16) only, a b3 >= 16 the three tiles with b1's tile <=
// b2's (the fourth holds b1 > b2 only) -- every cube is read once in either case.  Shells nb .. 16 NT - 1 are zero rows of
// the staging buffer, not reads; their tiles are formed like the others (a branch on b3 < nb inside the loop makes the
// compiler move every accumulator in and out of the AGPRs around each matrix instruction), so the time steps at nb = 16.
// EDGE: N^3 is not a multiple of FB_BK_RUN (N = 2 mod 4); voxels past the end are staged as zero.  A workgroup walks a
// contiguous range of runs in order and stores its accumulators to partial[workgroup][slot][256] (slot: b3 for b3 < 16,
// 16 + 3 (b3 - 16) + tile beyond; within a tile row-major b1, b2): fixed order, no atomics.
typedef double fb_bk_d4 __attribute__((ext_vector_type(4)));

template <typename T, int NT, bool EDGE>
__global__ __launch_bounds__(256)
void k_bk_contract(const T* __restrict__ cubes, long long stride, long long nvox, int nb, long long nruns,
                   double* __restrict__ partial) {
    constexpr int NBP = 16 * NT, LD = NBP + 1, PER = NBP / 4, NSLOT = NT == 1 ? 16 : 64;
    __shared__ double s[FB_BK_RUN * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
    const long long per = (nruns + gridDim.x - 1) / gridDim.x;
    const long long r0 = (long long)blockIdx.x * per, r1 = r0 + per < nruns ? r0 + per : nruns;
    fb_bk_d4 lo[4], hi[NT == 2 ? 4 : 1][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) lo[q] = fb_bk_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < (NT == 2 ? 4 : 1); ++q)
#pragma unroll
        for (int t = 0; t < 3; ++t) hi[q][t] = fb_bk_d4{0.0, 0.0, 0.0, 0.0};
    T g[PER];                                                          // shell wave + 4 q at voxel lane of a run
    auto fetch = [&](long long run) {
        const long long x = run * FB_BK_RUN + lane;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int b = wave + 4 * q;
            g[q] = (b < nb && (!EDGE || x < nvox)) ? cubes[(long long)b * stride + x] : (T)0;
        }
    };
    if (r0 < r1) fetch(r0);
    for (long long run = r0; run < r1; ++run) {
        __syncthreads();                                               // the previous run has been consumed
#pragma unroll
        for (int q = 0; q < PER; ++q) s[lane * LD + wave + 4 * q] = (double)g[q];
        __syncthreads();
        if (run + 1 < r1) fetch(run + 1);
#pragma unroll 4
        for (int ks = 0; ks < FB_BK_RUN / 4; ++ks) {
            const double* sx = s + (4 * ks + lk) * LD;
            const double v0 = sx[lc];
            const double v1 = NT == 2 ? sx[16 + lc] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                lo[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v0 * sx[wave + 4 * q], v0, lo[q], 0, 0, 0);
            if (NT == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double c = sx[16 + wave + 4 * q], a0 = v0 * c, a1 = v1 * c;
                    hi[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, v0, hi[q][0], 0, 0, 0);
                    hi[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, v1, hi[q][1], 0, 0, 0);
                    hi[q][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, v1, hi[q][2], 0, 0, 0);
                }
            }
        }
    }
    // D: col = lane & 15, row = (lane >> 4) + 4 reg, so [reg][lane] is the tile in row-major order
    double* dst = partial + (size_t)blockIdx.x * NSLOT * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b3 = wave + 4 * q;
        if (b3 < nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)b3 * 256 + 64 * r + lane] = lo[q][r];
        }
    }
    if (NT == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int b3 = 16 + wave + 4 * q;
            if (b3 < nb) {
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(size_t)(16 + 3 * (b3 - 16) + t) * 256 + 64 * r + lane] = hi[q][t][r];
            }
        }
    }
}

// out[t] = sum over the workgroups, in order, of the entry (b1, b2) of triple t's slot; t in
// itertools.combinations_with_replacement(range(nb), 3) order.  One workgroup per (b1 nb + b2, b3).
__global__ __launch_bounds__(256)
void k_bk_finish(const double* __restrict__ partial, int nblocks, int nslot, int nb, double* __restrict__ out) {
    __shared__ double sh[256];
    const int b1 = blockIdx.x / nb, b2 = blockIdx.x % nb, b3 = blockIdx.y;
    if (b1 > b2 || b2 > b3) return;
    int slot = b3, r = b1, c = b2;
    if (b3 >= 16) {
        const int tile = b1 < 16 ? (b2 < 16 ? 0 : 1) : 2;
        slot = 16 + 3 * (b3 - 16) + tile;
        r = b1 & 15; c = b2 & 15;
    }
    const double* src = partial + (size_t)slot * 256 + r * 16 + c;
    double v = 0.0;
    for (int q = threadIdx.x; q < nblocks; q += 256) v += src[(size_t)q * nslot * 256];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int t = 0;
        for (int q = 0; q < b1; ++q) t += (nb - q) * (nb - q + 1) / 2;   // triples that start below b1
        for (int q = b1; q < b2; ++q) t += nb - q;                      // (b1, q, *)
        out[t + (b3 - b2)] = sh[0];
    }
}

template <typename T>
int bk_split_launch(fb_plan* p, bool unit, const void* half, void* shells, const BkSplitArgs& a, double* partial,
                    double* out_dev, hipStream_t s) {
    const long long rows = (long long)p->N * p->NR;
    const int blocks = (int)std::max(1LL, std::min((rows + 3) / 4, 4LL * p->num_cu));
    const long long stride = (long long)p->N * p->NR * p->NZP;
    { FbProfScope _ps(p, FBK_BIN, s);
    if (unit)
        hipLaunchKernelGGL((k_bk_split<T, true>), dim3(blocks), dim3(256), 0, s, (const cx<T>*)half, (cx<T>*)shells, stride,
                           partial, a);
    else
        hipLaunchKernelGGL((k_bk_split<T, false>), dim3(blocks), dim3(256), 0, s, (const cx<T>*)half, (cx<T>*)shells, stride,
                           partial, a); }
    FB_LAUNCH_CHECK("k_bk_split");
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_bin_finish<>, dim3(3 * a.nq), dim3(256), 0, s, partial, blocks, 3 * a.nq, out_dev); }
    FB_LAUNCH_CHECK("k_bin_finish");
    return FB_OK;
}

// workgroups of the contraction: as many per CU as its registers admit (four with one tile per third shell, two with the 128
// accumulator registers of two tiles), never more than there are runs
int bk_contract_blocks(const fb_plan* p, long long nruns, int nb) {
    return (int)std::max(1LL, std::min(nruns, (nb <= 16 ? 4LL : 2LL) * p->num_cu));
}

template <typename T>
int bk_contract_launch(fb_plan* p, const void* cubes, int nb, double* partial, double* out_dev, hipStream_t s) {
    const long long nvox = (long long)p->N * p->N * p->N;
    const long long nruns = (nvox + FB_BK_RUN - 1) / FB_BK_RUN;
    const bool edge = nvox % FB_BK_RUN != 0;
    const int blocks = bk_contract_blocks(p, nruns, nb);
    const int nslot = nb <= 16 ? 16 : 64;
    { FbProfScope _ps(p, FBK_PCA, s);
#define FB_BK_GO(NT, EDGE) hipLaunchKernelGGL((k_bk_contract<T, NT, EDGE>), dim3(blocks), dim3(256), 0, s, (const T*)cubes, \
                                              nvox, nvox, nb, nruns, partial)
    if (nb <= 16) { if (edge) FB_BK_GO(1, true); else FB_BK_GO(1, false); }
    else { if (edge) FB_BK_GO(2, true); else FB_BK_GO(2, false); }
#undef FB_BK_GO
    }
    FB_LAUNCH_CHECK("k_bk_contract");
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_bk_finish, dim3(nb * nb, nb), dim3(256), 0, s, partial, blocks, nslot, nb, out_dev); }
    FB_LAUNCH_CHECK("k_bk_finish");
    return FB_OK;
}

int bk_check(const fb_plan* p, const double* kedges, int nb, int nwork) {
    FB_REQUIRE(nb >= 1 && nb <= FB_BK_MAX_SHELLS, "nb must be in 1..32");
    FB_REQUIRE(nwork >= 1 && nwork <= FB_BK_SPLIT, "nwork must be in 1..4");
    FB_REQUIRE(p->N <= 1024, "the bispectrum takes grids up to 1024^3");
    return kshell_check_edges(kedges, nb);
}

int bispectrum(fb_plan* p, const void* real, void* work_half, void* work_shells, int nwork, void* cubes, const double* kedges,
               int nb, int unit, double* out_host, hipStream_t s) {
    const int T3 = nb * (nb + 1) * (nb + 2) / 6;                       // <= 5984; with 3 nb shell sums within FB_SCRATCH
    const long long nvox = (long long)p->N * p->N * p->N;
    const long long rows = (long long)p->N * p->NR;
    const size_t half_bytes = (size_t)rows * p->NZP * 2 * p->prec, real_bytes = (size_t)nvox * p->prec;
    const size_t split_need = (size_t)std::max(1LL, std::min((rows + 3) / 4, 4LL * p->num_cu)) * 3 * FB_BK_SPLIT;
    const size_t con_need = (size_t)bk_contract_blocks(p, (nvox + FB_BK_RUN - 1) / FB_BK_RUN, nb) * (nb <= 16 ? 16 : 64) * 256;
    int r = p->work.ensure(std::max(split_need, con_need) * sizeof(double));
    if (r) return r;
    double* partial = p->work.as<double>();
    if (!unit) {
        r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real, work_half, 0, s), fbi_fft_r2c_f64(p, real, work_half, 0, s));
        if (r) return r;
    }
    BkSplitArgs a;
    for (int q = 0; q <= nb; ++q) a.thr[q] = sq_threshold(kedges[q]);
    for (int q = nb + 1; q <= FB_BK_MAX_SHELLS; ++q) a.thr[q] = INFINITY;
    fill_kf(p, a.kf);
    a.N = p->N; a.NZV = p->NZV; a.NZP = p->NZP; a.NR = p->NR; a.nb = nb;
    for (int b0 = 0; b0 < nb; b0 += nwork) {
        a.b0 = b0; a.nq = std::min(nwork, nb - b0);
        double* sums = p->scratch + T3 + 3 * b0;                       // [value][shell of the batch]
        r = FB_DISPATCH(p, bk_split_launch<float>(p, unit != 0, work_half, work_shells, a, partial, sums, s),
                        bk_split_launch<double>(p, unit != 0, work_half, work_shells, a, partial, sums, s));
        if (r) return r;
        for (int q = 0; q < a.nq; ++q) {                               // I_b = the unnormalised inverse transform of the shell
            void* sh = (char*)work_shells + (size_t)q * half_bytes;
            void* cube = (char*)cubes + (size_t)(b0 + q) * real_bytes;
            r = FB_DISPATCH(p, fbi_fft_c2r_f32(p, sh, cube, 1.0, s), fbi_fft_c2r_f64(p, sh, cube, 1.0, s));
            if (r) return r;
        }
    }
    r = FB_DISPATCH(p, bk_contract_launch<float>(p, cubes, nb, partial, p->scratch, s),
                    bk_contract_launch<double>(p, cubes, nb, partial, p->scratch, s));
    if (r) return r;
    std::vector<double> rec((size_t)T3 + 3 * nb);
    FB_TRY(fb_read_back(rec.data(), p->scratch, rec.size() * sizeof(double), s));
    std::copy(rec.begin(), rec.begin() + T3, out_host);
    for (int b0 = 0; b0 < nb; b0 += nwork) {
        const int nq = std::min(nwork, nb - b0);
        for (int v = 0; v < 3; ++v)
            for (int q = 0; q < nq; ++q) out_host[T3 + v * nb + b0 + q] = rec[(size_t)T3 + 3 * b0 + v * nq + q];
    }
    return FB_OK;
}

}  // namespace
}  // namespace fb

extern "C" {

int fb_bispectrum(fb_plan* p, const void* real, void* work_half, void* work_shells, int nwork, void* cubes,
                  const double* kedges, int nb, int unit, double* out_host, void* stream) {
    FB_REQUIRE(p && work_shells && cubes && kedges && out_host, "null pointer");
    FB_REQUIRE(unit || (real && work_half), "null pointer");
    const int r = fb::bk_check(p, kedges, nb, nwork);
    if (r) return r;
    FB_USE_DEVICE(p);
    return fb::bispectrum(p, real, work_half, work_shells, nwork, cubes, kedges, nb, unit, out_host, (hipStream_t)stream);
}

int fb_device_memory(int64_t* free_bytes, int64_t* total_bytes) {
    FB_REQUIRE(free_bytes && total_bytes, "null pointer");
    size_t f = 0, t = 0;
    FB_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f; *total_bytes = (int64_t)t;
    return FB_OK;
}

}  // extern "C"
