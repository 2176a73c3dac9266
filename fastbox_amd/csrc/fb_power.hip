// Power spectrum in (k, mu) bins with multipoles (nbodykit FFTPower(mode='1d' | '2d', los=[0,0,1]) on a mesh): the binning of
// Re(conj(D_1) D_2) straight from one or two stored half spectra.  Both plan precisions are compiled here; see
// include/fastbox_hip.h for the definition and DESIGN.md section 4 for the algorithm and its limits.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"                      // mode_of, wave_sum, k_bin_finish
#include "fb_fft.h"                      // cx<T>
#include "fb_kshell.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace fb {
namespace {

// A mode's cell is decided with the fp64 expressions of the definition without forming |k| or mu in most cases:
//   |k| bin: digitize(sqrt(k2), e) = #{b : T_b <= k2} with T_b the least double whose correctly rounded sqrt reaches e_b
//            (host, fp64 std::sqrt); a float guess of the bin is corrected with those exact comparisons;
//   mu bin : mu = |k_z| / sqrt(k2) against linspace(0, 1, nmu + 1); a float estimate decides unless it lies within 1e-3
//            of a bin's width from an interior edge, where the fp64 expression itself is evaluated.
struct PkArgs {
    const double* tab;     // [nk + 1] thresholds T_b, then [nmu + 1] mu edges
    int N, NZV, NZP, NR;
    int nk, nmu, nv;       // nv: values per cell (data: 1 + lmax / 2; geometry: 1, selected by which)
    int which;             // geometry pass: 0 modes, 1 sum |k|, 2 sum mu
    int uniform;           // edges evenly spaced: e0 + b dk (only the guess uses it)
    float e0f, inv_dkf;
    double kf[3];          // 2 pi / L_a
};

#define FB_PK_WAVES 4      // waves per workgroup when the per-wave rows fit (fewer otherwise: pk_waves)
#define FB_PK_GROUP 4      // 64-lane steps whose loads a wave issues together (a row of N <= 512 is two groups)

// -1 below the first edge, nk at or beyond the last one
__device__ __forceinline__ int pk_kbin(const double* T, const PkArgs& a, double k2) {
    const int nk = a.nk;
    int b;
    if (a.uniform) {
        const float t = (sqrtf((float)k2) - a.e0f) * a.inv_dkf;
        b = t < 0.f ? -1 : (t >= (float)nk ? nk : (int)t);
    } else {
        int lo = 0, hi = nk + 1;                                     // number of thresholds <= k2
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (T[mid] <= k2) lo = mid + 1; else hi = mid; }
        b = lo - 1;
    }
    while (b >= 0 && T[b] > k2) --b;
    while (b < nk && T[b + 1] <= k2) ++b;
    return b;
}
__device__ __forceinline__ int pk_mubin(const double* me, const PkArgs& a, double kz, double k2) {
    const int nmu = a.nmu;
    if (nmu == 1) return 0;
    const float t = fabsf((float)kz) * rsqrtf((float)k2) * (float)nmu;
    if (t < 0.5f) return 0;                                          // (every mu >= 0 = the first edge)
    if (t > (float)nmu - 0.5f) return nmu - 1;                       // mu == 1 (or a rounding above) joins the last bin
    if (fabsf(t - rintf(t)) > 1e-3f) return (int)t;
    const double mu = fabs(kz) / sqrt(k2);
    int c = 0;
    for (int q = 1; q <= nmu; ++q) c += me[q] <= mu ? 1 : 0;
    return c < nmu - 1 ? c : nmu - 1;
}

// One (k_x, k_y) row of the half spectrum per wave, lanes along k_z (l = lane, lane + 64, ...).  Along a row k2 and mu both
// grow with l, so the cell key = kbin nmu + mubin never decreases over the lanes of a step: a step inside one cell takes plain
// wave sums, otherwise a segmented scan leaves each cell's sum in the last lane of its run and those lanes (distinct cells)
// add into the wave's LDS row.  Lanes below the first edge (and k = 0) carry key -1, lanes beyond the last edge or the row
// key INT_MAX: they are runs that write nothing.  Rows with k_perp^2 >= T_nk are skipped, a row stops at the first step
// that starts beyond the last edge.  Per-workgroup partials [value][workgroup], then k_bin_finish: fixed order, no atomics.
template <typename T, bool GEOM>
__global__ __launch_bounds__(64 * FB_PK_WAVES)
void k_pk_bin(const cx<T>* __restrict__ h1, const cx<T>* __restrict__ h2, double* __restrict__ partial, PkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nk = a.nk, nmu = a.nmu, nc = nk * nmu, nv = a.nv, N = a.N;
    const int waves = blockDim.x >> 6;
    double* tk = reinterpret_cast<double*>(smem);
    double* me = tk + nk + 1;
    double* acc = me + nmu + 1;                                      // [waves][nv][nc]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < nk + nmu + 2; q += blockDim.x) tk[q] = a.tab[q];
    for (int q = tid; q < waves * nv * nc; q += blockDim.x) acc[q] = 0.0;
    __syncthreads();
    double* row_acc = acc + (size_t)wave * nv * nc;
    const double tlast = tk[nk];
    const long long nrows = (long long)N * N;
    for (long long row = (long long)blockIdx.x * waves + wave; row < nrows; row += (long long)gridDim.x * waves) {
        const int i = (int)(row / N), j = (int)(row % N);
        const double kperp2 = sq2((double)mode_of(i, N) * a.kf[0], (double)mode_of(j, N) * a.kf[1]);
        if (kperp2 >= tlast) continue;                               // the whole row lies beyond the last edge
        const long long base = ((long long)i * a.NR + j) * a.NZP;
        bool done = false;
        for (int g0 = 0; g0 < a.NZV && !done; g0 += 64 * FB_PK_GROUP) {
            cx<T> d1[FB_PK_GROUP], d2[FB_PK_GROUP];
            if (!GEOM) {
#pragma unroll
                for (int c = 0; c < FB_PK_GROUP; ++c) {               // all loads of the group first
                    const int l = g0 + 64 * c + lane;
                    d1[c] = l < a.NZV ? h1[base + l] : cx<T>{0, 0};
                    d2[c] = (h2 && l < a.NZV) ? h2[base + l] : d1[c];
                }
            }
#pragma unroll
            for (int c = 0; c < FB_PK_GROUP; ++c) {
                const int l0 = g0 + 64 * c, l = l0 + lane;
                if (l0 >= a.NZV) { done = true; break; }
                const double kz = (double)l * a.kf[2];               // l <= N / 2: the stored k_z are the non-negative ones
                const double k2 = add_sq(kperp2, kz);
                if (__shfl(k2, 0, 64) >= tlast) { done = true; break; }   // lane 0 beyond the last edge: so is the rest
                const bool in = l < a.NZV && k2 > 0.0;
                int key = 0x7fffffff;
                if (in) {
                    const int kb = pk_kbin(tk, a, k2);
                    key = kb < 0 ? -1 : (kb >= nk ? 0x7fffffff : kb * nmu + pk_mubin(me, a, kz, k2));
                } else if (l < a.NZV) key = -1;                      // k = 0
                const bool ok = key >= 0 && key < nc;
                const double w = !ok ? 0.0 : ((l == 0 || 2 * l == N) ? 1.0 : 2.0);
                double v[3] = {0.0, 0.0, 0.0};
                if (GEOM) {
                    if (ok) v[0] = a.which == 0 ? w : (a.which == 1 ? w * sqrt(k2) : w * (kz / sqrt(k2)));
                } else {
                    const double p = (double)d1[c].x * (double)d2[c].x + (double)d1[c].y * (double)d2[c].y;
                    v[0] = w * p;
                    if (nv > 1) {
                        const double m2 = ok ? (kz * kz) / k2 : 0.0;
                        v[1] = v[0] * (1.5 * m2 - 0.5);
                        v[2] = v[0] * (((35.0 * m2 - 30.0) * m2 + 3.0) * 0.125);
                    }
                }
                const int kfirst = __shfl(key, 0, 64), klast = __shfl(key, 63, 64);
                if (kfirst == klast) {                               // fast path: the step lies in one cell (or none)
                    if (kfirst >= 0 && kfirst < nc) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            if (q >= nv) break;
                            const double s = wave_sum(v[q]);
                            if (lane == 0) row_acc[q * nc + kfirst] += s;
                        }
                    }
                } else {
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {              // segmented inclusive scan over runs of equal keys
                        const int ko = __shfl_up(key, o, 64);
                        const bool same = lane >= o && ko == key;
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            if (q >= nv) break;
                            const double s = __shfl_up(v[q], o, 64);
                            if (same) v[q] += s;
                        }
                    }
                    const int kn = __shfl_down(key, 1, 64);
                    if (ok && (lane == 63 || kn != key)) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) if (q < nv) row_acc[q * nc + key] += v[q];
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < nv * nc; q += blockDim.x) {
        double s = 0.0;
        for (int w = 0; w < waves; ++w) s += acc[(size_t)w * nv * nc + q];
        partial[(size_t)q * gridDim.x + blockIdx.x] = s;             // [value][workgroup]: see k_bin_finish
    }
}

template <typename T> struct PkKernels {
    static const void* geom() { return reinterpret_cast<const void*>(k_pk_bin<T, true>); }
    static const void* data() { return reinterpret_cast<const void*>(k_pk_bin<T, false>); }
};

// LDS of a workgroup of `waves` waves; the largest per-wave row (nk nmu nv <= FB_PK_MAX_VALUES doubles, 40 KiB) leaves room
// for three waves in the CU's 160 KiB, anything up to 2 x 1024 x 3 values for four
size_t pk_lds(int nk, int nmu, int nv, int waves) {
    return (size_t)(nk + nmu + 2) * 8 + (size_t)waves * nv * nk * nmu * 8;
}
int pk_waves(int nk, int nmu, int nv) {
    for (int w = FB_PK_WAVES; w > 1; --w) if (pk_lds(nk, nmu, nv, w) <= 160 * 1024) return w;
    return 1;
}

// out_dev[nv][nk nmu]: the sums of one binning pass (GEOM: the value `which` only, nv = 1)
template <typename T>
int pk_launch(fb_plan* p, bool geom, int which, const void* h1, const void* h2, const PkArgs& base, double* out_dev,
              hipStream_t s) {
    PkArgs a = base;
    a.which = which;
    const int nc = a.nk * a.nmu;
    const int waves = pk_waves(a.nk, a.nmu, a.nv);
    const size_t lds = pk_lds(a.nk, a.nmu, a.nv, waves);
    const long long rows = (long long)p->N * p->N;
    const long long resident = std::max(1LL, std::min(8LL, (long long)((160 * 1024) / lds)));   // workgroups per CU
    long long blocks = std::min((rows + waves - 1) / waves, resident * p->num_cu);
    if (blocks < 1) blocks = 1;
    FB_TRY(p->pk_partials.ensure((size_t)blocks * a.nv * nc * sizeof(double)));
    const void* fn = geom ? PkKernels<T>::geom() : PkKernels<T>::data();
    if (lds > 65536) FB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    { FbProfScope _ps(p, FBK_BIN, s);
    if (geom)
        hipLaunchKernelGGL((k_pk_bin<T, true>), dim3((unsigned)blocks), dim3(64 * waves), lds, s, (const cx<T>*)h1,
                           (const cx<T>*)h2, p->pk_partials, a);
    else
        hipLaunchKernelGGL((k_pk_bin<T, false>), dim3((unsigned)blocks), dim3(64 * waves), lds, s, (const cx<T>*)h1,
                           (const cx<T>*)h2, p->pk_partials, a); }
    FB_LAUNCH_CHECK("k_pk_bin");
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_bin_finish<>, dim3(a.nv * nc), dim3(256), 0, s, p->pk_partials, (int)blocks, a.nv * nc, out_dev); }
    FB_LAUNCH_CHECK("k_bin_finish");
    return FB_OK;
}

int pk_check(const double* kedges, int nk, int nmu, int lmax) {
    FB_REQUIRE(nk >= 1 && nk <= FB_PK_MAX_K, "nk must be in 1..1024");
    FB_REQUIRE(nmu >= 1 && nmu <= FB_PK_MAX_MU, "nmu must be in 1..128");
    FB_REQUIRE(lmax == 0 || lmax == 2 || lmax == 4, "lmax must be 0, 2 or 4");
    FB_REQUIRE((long long)nk * nmu * (lmax / 2 + 1) <= FB_PK_MAX_VALUES, "nk * nmu * (lmax / 2 + 1) must be <= 5120");
    return kshell_check_edges(kedges, nk);
}

int bin_power_kmu(fb_plan* p, const void* half1, const void* half2, const double* kedges, int nk, int nmu, int lmax,
                  double* out_host, hipStream_t s) {
    const int nc = nk * nmu, nl = lmax / 2 + 1;
    // device table: thresholds in k^2, then numpy's linspace(0, 1, nmu + 1) (arange * (1 / nmu) + 0, last = 1)
    std::vector<double> tab(nk + nmu + 2);
    for (int q = 0; q <= nk; ++q) tab[q] = sq_threshold(kedges[q]);
    const double step = 1.0 / nmu;
    for (int q = 0; q <= nmu; ++q) tab[nk + 1 + q] = (double)q * step + 0.0;
    tab[nk + 1 + nmu] = 1.0;
    FB_TRY(p->pk_tab.ensure((FB_PK_MAX_K + FB_PK_MAX_MU + 2) * sizeof(double)));
    FB_HIP(hipMemcpyAsync(p->pk_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    PkArgs a;
    a.tab = p->pk_tab; a.N = p->N; a.NZV = p->NZV; a.NZP = p->NZP; a.NR = p->NR;
    a.nk = nk; a.nmu = nmu; a.nv = nl; a.which = 0;
    fill_kf(p, a.kf);
    const double dk = (kedges[nk] - kedges[0]) / nk;
    bool uni = std::isfinite(dk) && dk > 0.0;
    for (int q = 0; uni && q <= nk; ++q) uni = std::fabs(kedges[q] - (kedges[0] + q * dk)) <= 1e-6 * dk;
    a.uniform = uni ? 1 : 0;
    a.e0f = (float)kedges[0];
    a.inv_dkf = uni ? (float)(1.0 / dk) : 0.f;
    // the data-independent sums: once per (edges, nmu)
    std::vector<double> key(kedges, kedges + nk + 1);
    key.push_back((double)nmu);
    const std::vector<double>* geo = p->pk_geom.find(key);
    if (!geo) {
        std::vector<double> e(3 * (size_t)nc);
        PkArgs g = a;
        g.nv = 1;
        for (int w = 0; w < 3; ++w) {
            int r = FB_DISPATCH(p, pk_launch<float>(p, true, w, nullptr, nullptr, g, p->scratch, s),
                                pk_launch<double>(p, true, w, nullptr, nullptr, g, p->scratch, s));
            if (r) return r;
            FB_TRY(fb_read_back(e.data() + (size_t)w * nc, p->scratch, (size_t)nc * sizeof(double), s));
        }
        geo = p->pk_geom.insert(key, std::move(e));
    }
    int r = FB_DISPATCH(p, pk_launch<float>(p, false, 0, half1, half2, a, p->scratch, s),
                        pk_launch<double>(p, false, 0, half1, half2, a, p->scratch, s));
    if (r) return r;
    std::vector<double> sums((size_t)nl * nc);
    FB_TRY(fb_read_back(sums.data(), p->scratch, sums.size() * sizeof(double), s));
    std::copy(geo->begin(), geo->end(), out_host);
    // P = (Lx Ly Lz / N^6) Re(conj(D_1) D_2)
    const double n3 = (double)p->N * p->N * p->N;
    const double scale = (p->L[0] * p->L[1] * p->L[2]) / (n3 * n3);
    for (int q = 0; q < nc; ++q) out_host[3 * nc + q] = sums[q] * scale;
    for (int l = 1; l < nl; ++l)                                     // sum P L_l per k bin: the mu cells in order
        for (int b = 0; b < nk; ++b) {
            double t = 0.0;
            for (int c = 0; c < nmu; ++c) t += sums[(size_t)l * nc + (size_t)b * nmu + c];
            out_host[4 * nc + (size_t)(l - 1) * nk + b] = t * scale;
        }
    return FB_OK;
}

}  // namespace
}  // namespace fb

extern "C" {

int fb_bin_power_kmu(fb_plan* p, const void* half1, const void* half2, const double* kedges, int nk, int nmu, int lmax,
                     double* out_host, void* stream) {
    FB_REQUIRE(p && half1 && kedges && out_host, "null pointer");
    const int r = fb::pk_check(kedges, nk, nmu, lmax);
    if (r) return r;
    FB_USE_DEVICE(p);
    return fb::bin_power_kmu(p, half1, half2, kedges, nk, nmu, lmax, out_host, (hipStream_t)stream);
}

int fb_power_spectrum_kmu(fb_plan* p, const void* real1, const void* real2, void* work_half1, void* work_half2,
                          const double* kedges, int nk, int nmu, int lmax, double* out_host, void* stream) {
    FB_REQUIRE(p && real1 && work_half1 && kedges && out_host, "null pointer");
    FB_REQUIRE(!real2 || work_half2, "a cross spectrum needs work_half2");
    int r = fb::pk_check(kedges, nk, nmu, lmax);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real1, work_half1, 0, s), fbi_fft_r2c_f64(p, real1, work_half1, 0, s));
    if (!r && real2) r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real2, work_half2, 0, s), fbi_fft_r2c_f64(p, real2, work_half2, 0, s));
    if (r) return r;
    return fb::bin_power_kmu(p, work_half1, real2 ? work_half2 : nullptr, kedges, nk, nmu, lmax, out_host, s);
}

}  // extern "C"
