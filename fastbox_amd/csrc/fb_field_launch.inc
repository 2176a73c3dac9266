// Host launchers of the element-wise kernels for one precision (FB_REAL / FB_SUFFIX).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_field_kernels.h"
#include <vector>

namespace {
using namespace fb;
typedef FB_REAL real_t;
typedef cx<real_t> cplx_t;

KGeom geom(const fb_plan* p) { return KGeom{p->axis2, p->ksc, p->kpar, p->N, p->NZV, p->NZP, p->NR}; }
BinGeom bin_geom(const fb_plan* p) {
    BinGeom b;
    b.bins = p->bins; b.thr = p->use_thr ? p->thr : nullptr; b.nbins = p->nbins; b.namb = p->namb;
    for (int q = 0; q < 8; ++q) b.amb[q] = p->amb[q];
    return b;
}
dim3 mode_grid(const fb_plan* p, int nz, int bs) { return dim3((nz + bs - 1) / bs, p->N, p->N); }
RngKey rng_key(uint64_t seed, uint64_t real) {
    RngKey k;
    k.k[0] = (uint32_t)seed; k.k[1] = (uint32_t)(seed >> 32); k.k[2] = (uint32_t)real; k.k[3] = (uint32_t)(real >> 32);
    return k;
}
dim3 row_grid(const fb_plan* p) {      // one (k_x, k_y) row per 64 lanes
    return dim3((unsigned)(((long long)p->N * p->N + FB_ROW_GROUPS - 1) / FB_ROW_GROUPS));
}
int mode_block(int nz) {                 // threads along k_z: least padding (N/2 + 1 columns -> 64), ties to the larger
    int best = 64;
    for (int bs = 128; bs <= 256; bs <<= 1)
        if ((nz + bs - 1) / bs * bs <= (nz + best - 1) / best * best) best = bs;
    return best;
}

int amp_src(const fb_plan* p, AmpSrc<real_t>& a) {
    a.shell = p->amp_shell.as<const real_t>();
    a.dense = reinterpret_cast<const real_t*>(p->amp_dense);
    a.sym = p->amp_sym.as<const real_t>();
    if (a.dense) a.shell = nullptr;
    if (p->amp_sym_only) { a.shell = nullptr; a.dense = nullptr; }
    if (!a.shell && !a.dense && !a.sym) { fb_set_error("amplitude table not set (fb_set_amplitude_*)"); return FB_ERR_STATE; }
    return FB_OK;
}
}  // namespace

#define FB_CAT2(a, b) a##b
#define FB_CAT(a, b) FB_CAT2(a, b)
#define FBI(name) FB_CAT(FB_CAT(fbi_, name), FB_CAT(_, FB_SUFFIX))

int FBI(set_amp_shells)(fb_plan* p, const double* amp, int64_t n) {
    std::vector<real_t> tmp((size_t)n);
    for (int64_t q = 0; q < n; ++q) tmp[(size_t)q] = (real_t)amp[q];
    FB_TRY(p->amp_shell.reset());
    FB_TRY(p->amp_shell.ensure((size_t)n * sizeof(real_t)));
    FB_HIP(hipMemcpy(p->amp_shell, tmp.data(), (size_t)n * sizeof(real_t), hipMemcpyHostToDevice));
    p->nshell = n;
    p->amp_sym_only = 0;
    // the generator's k_z-contiguous copy (see k_build_amp_sym); FB_NO_AMP_SYM=1 keeps only the shell table
    const int N = p->N, M = N / 2 + 1;
    if (const char* e = getenv("FB_NO_AMP_SYM")) if (e[0] == '1') {
        return p->amp_sym.reset();
    }
    if (n < (int64_t)3 * (N / 2) * (N / 2) + 1) { fb_set_error("shell table shorter than 3 (N/2)^2 + 1"); return FB_ERR_INVALID; }
    FB_TRY(p->amp_sym.ensure((size_t)M * M * p->NZP * sizeof(real_t)));
    hipLaunchKernelGGL((k_build_amp_sym<real_t>), dim3((p->NZP + 63) / 64, M, M), dim3(64), 0, 0,
                       p->amp_shell.as<const real_t>(), p->amp_sym.as<real_t>(), N, p->NZP);
    FB_LAUNCH_CHECK("k_build_amp_sym");
    FB_HIP(hipDeviceSynchronize());
    return FB_OK;
}

// Any box shape: amplitudes per (|m_x|, |m_y|, |m_z|), host double[M][M][M] with M = N/2 + 1 (|k| depends on the
// mode numbers only through their magnitudes), stored as the generator's k_z-contiguous table [M][M][NZP].
int FBI(set_amp_sym)(fb_plan* p, const double* amp, int64_t n) {
    const int N = p->N, M = N / 2 + 1;
    if (n != (int64_t)M * M * M) { fb_set_error("expected (N/2+1)^3 amplitudes"); return FB_ERR_INVALID; }
    std::vector<real_t> tmp((size_t)M * M * p->NZP, (real_t)0);
    for (int a = 0; a < M; ++a)
        for (int b = 0; b < M; ++b)
            for (int c = 0; c < M; ++c)
                tmp[((size_t)a * M + b) * p->NZP + c] = (real_t)amp[((size_t)a * M + b) * M + c];
    FB_TRY(p->amp_sym.ensure(tmp.size() * sizeof(real_t)));
    FB_HIP(hipMemcpy(p->amp_sym, tmp.data(), tmp.size() * sizeof(real_t), hipMemcpyHostToDevice));
    p->amp_sym_only = 1;
    p->amp_dense = nullptr;
    return FB_OK;
}

int FBI(colour_noise)(fb_plan* p, const void* re, const void* im, void* out, hipStream_t s) {
    AmpSrc<real_t> a;
    int r = amp_src(p, a);
    if (r) return r;
    const int bs = mode_block(p->NZV);
    { FbProfScope _ps(p, FBK_COLOUR, s);
    hipLaunchKernelGGL((k_colour_noise<real_t>), mode_grid(p, p->NZV, bs), dim3(bs), 0, s,
                       (const real_t*)re, (const real_t*)im, (cplx_t*)out, a, geom(p)); }
    FB_LAUNCH_CHECK("k_colour_noise");
    return FB_OK;
}

int FBI(colour_device)(fb_plan* p, uint64_t seed, uint64_t real, void* out, hipStream_t s) {
    AmpSrc<real_t> a;
    int r = amp_src(p, a);
    if (r) return r;
    const int bs = mode_block(p->NZV);
    { FbProfScope _ps(p, FBK_COLOUR, s);
    hipLaunchKernelGGL((k_colour_device<real_t>), mode_grid(p, p->NZV, bs), dim3(bs), 0, s, (cplx_t*)out, a, geom(p),
                       rng_key(seed, real)); }
    FB_LAUNCH_CHECK("k_colour_device");
    return FB_OK;
}

// sums_dev[2*nbins] <- (sum |dk|^2, sum |dk|^4) per bin over the full grid
namespace {
int filter_spec(FilterSpec& f, int kind, const double* prm, const void* table) {
    f.kind = kind;
    for (int q = 0; q < 4; ++q) f.p[q] = prm ? prm[q] : 0.0;
    f.table = table;
    if (kind == FILT_TABLE && !table) { fb_set_error("FB_FILT_TABLE needs a device table"); return FB_ERR_INVALID; }
    if (kind < 0 || kind > FILT_TOPHAT) { fb_set_error("unknown filter kind"); return FB_ERR_INVALID; }
    return FB_OK;
}
}  // namespace

// filter_kind < 0: plain |delta_k|^2; otherwise |delta_k T(k)|^2 without storing the filtered spectrum
int FBI(bin_power)(fb_plan* p, const void* half, int layout, int filter_kind, const double* prm, const void* table,
                   double* sums_dev, hipStream_t s) {
    if (!p->nbins) { fb_set_error("bin edges not set (fb_set_bins)"); return FB_ERR_STATE; }
    const int nb = p->nbins;
    FilterSpec f;
    f.kind = -1; f.table = nullptr;
    for (int q = 0; q < 4; ++q) f.p[q] = 0.0;
    if (filter_kind >= 0) { int r = filter_spec(f, filter_kind, prm, table); if (r) return r; }
    const size_t lds = (size_t)nb * 8 + (size_t)FB_BIN_WAVES * nb * 16 + (size_t)nb * 4;
    long long rows = (long long)p->N * p->N;
    int blocks = (int)((rows + FB_BIN_WAVES - 1) / FB_BIN_WAVES);
    if (blocks > p->prow) blocks = p->prow;
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL((k_bin_rows<real_t>), dim3(blocks), dim3(64 * FB_BIN_WAVES), lds, s, (const cplx_t*)half,
                       p->partials, geom(p), bin_geom(p), f, layout ? 0 : 1); }
    FB_LAUNCH_CHECK("k_bin_rows");
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_bin_finish<>, dim3(2 * nb), dim3(256), 0, s, p->partials, blocks, 2 * nb, sums_dev); }
    FB_LAUNCH_CHECK("k_bin_finish");
    return FB_OK;
}

int FBI(apply_filter)(fb_plan* p, const void* in, void* out, int layout, int kind, const double* prm,
                      const void* table, hipStream_t s) {
    FilterSpec f;
    int r = filter_spec(f, kind, prm, table);
    if (r) return r;
    const int nz = layout ? p->NZV : p->N, pitch = layout ? p->NZP : p->N;
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_apply_filter<real_t>), row_grid(p), dim3(64, FB_ROW_GROUPS), 0, s, (const cplx_t*)in, (cplx_t*)out,
                       f, geom(p), pitch, nz); }
    FB_LAUNCH_CHECK("k_apply_filter");
    return FB_OK;
}

int FBI(velocity)(fb_plan* p, const void* dk, void* out, int layout, int comp, double fac, hipStream_t s) {
    if (comp < 0 || comp > 2) { fb_set_error("component must be 0, 1 or 2"); return FB_ERR_INVALID; }
    const int nz = layout ? p->NZV : p->N, pitch = layout ? p->NZP : p->N;
    { FbProfScope _ps(p, FBK_VELPOT, s);
    hipLaunchKernelGGL((k_velocity<real_t>), row_grid(p), dim3(64, FB_ROW_GROUPS), 0, s, (const cplx_t*)dk, (cplx_t*)out,
                       geom(p), comp, fac, pitch, nz); }
    FB_LAUNCH_CHECK("k_velocity");
    return FB_OK;
}

int FBI(potential)(fb_plan* p, const void* dk, void* out, int layout, hipStream_t s) {
    const int nz = layout ? p->NZV : p->N, pitch = layout ? p->NZP : p->N;
    { FbProfScope _ps(p, FBK_VELPOT, s);
    hipLaunchKernelGGL((k_potential<real_t>), row_grid(p), dim3(64, FB_ROW_GROUPS), 0, s, (const cplx_t*)dk, (cplx_t*)out,
                       geom(p), pitch, nz); }
    FB_LAUNCH_CHECK("k_potential");
    return FB_OK;
}

namespace {
int finish_partials(fb_plan* p, int nblocks, double* out, hipStream_t s) {
    std::vector<double> h((size_t)nblocks);
    FB_TRY(fb_read_back(h.data(), p->scratch, (size_t)nblocks * sizeof(double), s));
    double t = 0.0;
    for (int q = 0; q < nblocks; ++q) t += h[(size_t)q];
    *out = t;
    return FB_OK;
}
int reduce_blocks(long long n) {
    long long b = (n + 256 * 8 - 1) / (256 * 8);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}
}  // namespace

namespace {
int finish_partials_max(fb_plan* p, int nblocks, double* out, hipStream_t s) {
    std::vector<double> h((size_t)nblocks);
    FB_TRY(fb_read_back(h.data(), p->scratch, (size_t)nblocks * sizeof(double), s));
    double t = h[0];
    for (int q = 1; q < nblocks; ++q) t = h[(size_t)q] > t ? h[(size_t)q] : t;
    *out = t;
    return FB_OK;
}
}  // namespace

// largest value of a real cube (the shift of a log-normal transform is taken from it)
int FBI(max_real)(fb_plan* p, const void* x, double* out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    const int nb = reduce_blocks(n);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_reduce_real<real_t, 3>), dim3(nb), dim3(256), 0, s, (const real_t*)x, (real_t*)nullptr, n,
                       p->scratch, 0.0); }
    FB_LAUNCH_CHECK("k_reduce_real<max>");
    return finish_partials_max(p, nb, out, s);
}

// exp(x)/mean(exp(x)) - 1 (box.py:457-460), formed as exp(x - max x) / mean(exp(x - max x)) - 1: the same numbers, and
// nothing overflows whatever the field's variance (a single-precision exp(x) is infinite from x = 88.8: 6 sigma of the
// non-linear field of a 2048^3 box at 0.5 Mpc per voxel)
int FBI(lognormal)(fb_plan* p, const void* in, void* out, double* mean_out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    const int nb = reduce_blocks(n);
    double xmax = 0.0;
    int r = FBI(max_real)(p, in, &xmax, s);
    if (r) return r;
    if (!(xmax > -1e300 && xmax < 1e300)) xmax = 0.0;            // all-NaN or infinite input: exp() of it as it stands
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_reduce_real<real_t, 2>), dim3(nb), dim3(256), 0, s, (const real_t*)in, (real_t*)out, n,
                       p->scratch, xmax); }
    FB_LAUNCH_CHECK("k_reduce_real<exp>");
    double tot = 0.0;
    r = finish_partials(p, nb, &tot, s);
    if (r) return r;
    const double mean = tot / (double)n;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_affine<real_t>), dim3(nb), dim3(256), 0, s, (real_t*)out, n, (real_t)(1.0 / mean), (real_t)-1); }
    FB_LAUNCH_CHECK("k_affine");
    if (mean_out) *mean_out = mean * exp(xmax);                  // mean(exp(x)); may overflow a double for sigma >~ 100
    return FB_OK;
}

int FBI(rsd)(fb_plan* p, const void* d, const void* vz, const void* noise, void* out, double Hz, double sigma,
             uint64_t seed, int nearest, hipStream_t s) {
    const int N = p->N;
    const int bs = N >= 256 ? 256 : (N >= 128 ? 128 : 64);
    if (nearest != 2 && !p->generic && N >= 64 && N <= 2048) {      // one wavefront per line of sight, no sort (LDS: N*56 B f32, N*72 B f64)
        FbProfScope _ps(p, FBK_RSD, s);
#define FB_RSD_CASE(E_)                                                                                              \
        case E_ * 64: {                                                                                              \
            constexpr int W = rsd_waves(E_);                                                                         \
            const unsigned nb = (unsigned)((long long)N * N / W);                                                    \
            const size_t lds = (size_t)N * (8 + W * (sizeof(rsd_key<real_t>::type) + sizeof(real_t))) + W * 16 * sizeof(real_t); \
            if (lds > 65536)                                                                                         \
                FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rsd_cells<real_t, E_>),                    \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                   \
            hipLaunchKernelGGL((k_rsd_cells<real_t, E_>), dim3(nb), dim3(64 * W), lds, s, (const real_t*)d,          \
                               (const real_t*)vz, (const real_t*)noise, (real_t*)out, p->zgrid, Hz, sigma,           \
                               rng_key(seed, 0), nearest);                                                           \
            break; }
        switch (N) { FB_RSD_CASE(1) FB_RSD_CASE(2) FB_RSD_CASE(4) FB_RSD_CASE(8) FB_RSD_CASE(16) FB_RSD_CASE(32) }
#undef FB_RSD_CASE
        FB_LAUNCH_CHECK("k_rsd_cells");
        return FB_OK;
    }
    // (the sorting kernel: N < 64, and method 2 = the cubic spline of griddata(method='cubic') at any N: 32 bytes of LDS per point)
    int N2 = 1;
    while (N2 < N) N2 <<= 1;
    const size_t lds_rsd = (size_t)N2 * (nearest == 2 ? 32 : 16);
    if (lds_rsd > 65536)
        FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rsd<real_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rsd));
    { FbProfScope _ps(p, FBK_RSD, s);
    hipLaunchKernelGGL((k_rsd<real_t>), dim3((unsigned)((long long)N * N)), dim3(bs), lds_rsd, s,
                       (const real_t*)d, (const real_t*)vz, (const real_t*)noise, (real_t*)out, p->zgrid, N, Hz, sigma,
                       rng_key(seed, 0), nearest, N2); }
    FB_LAUNCH_CHECK("k_rsd");
    return FB_OK;
}

int FBI(sum_real)(fb_plan* p, const void* x, int squared, double* out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    const int nb = reduce_blocks(n);
    if (squared)
        { FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL((k_reduce_real<real_t, 1>), dim3(nb), dim3(256), 0, s, (const real_t*)x, (real_t*)nullptr, n,
                           p->scratch); }
    else
        { FbProfScope _ps(p, FBK_REALOP, s);
        hipLaunchKernelGGL((k_reduce_real<real_t, 0>), dim3(nb), dim3(256), 0, s, (const real_t*)x, (real_t*)nullptr, n,
                           p->scratch); }
    FB_LAUNCH_CHECK("k_reduce_real");
    return finish_partials(p, nb, out, s);
}

int FBI(sumsq_half)(fb_plan* p, const void* h, double* out, hipStream_t s) {
    const int nb = 1024;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_sumsq_half<real_t>), dim3(nb), dim3(256), 0, s, (const cplx_t*)h, geom(p), p->scratch); }
    FB_LAUNCH_CHECK("k_sumsq_half");
    return finish_partials(p, nb, out, s);
}

int FBI(expand_half)(fb_plan* p, const void* h, void* f, hipStream_t s) {
    const int bs = mode_block(p->N);
    { FbProfScope _ps(p, FBK_LAYOUT, s);
    hipLaunchKernelGGL((k_expand_half<real_t>), mode_grid(p, p->N, bs), dim3(bs), 0, s, (const cplx_t*)h, (cplx_t*)f,
                       geom(p)); }
    FB_LAUNCH_CHECK("k_expand_half");
    return FB_OK;
}

int FBI(crop_full)(fb_plan* p, const void* f, void* h, hipStream_t s) {
    const int bs = mode_block(p->NZV);
    { FbProfScope _ps(p, FBK_LAYOUT, s);
    hipLaunchKernelGGL((k_crop_full<real_t>), mode_grid(p, p->NZV, bs), dim3(bs), 0, s, (const cplx_t*)f, (cplx_t*)h,
                       geom(p)); }
    FB_LAUNCH_CHECK("k_crop_full");
    return FB_OK;
}

// ---- two-point correlation function (kernels: fb_field_kernels.h, k_cross_power / k_sep_bin) ------------------------
int FBI(cross_power)(fb_plan* p, const void* a, const void* b, void* out, double scale, hipStream_t s) {
    const long long n = (long long)p->N * p->NR * p->NZP;
    const long long blocks = std::min((n + 255) / 256, 8LL * p->num_cu * 8);          // 8 resident 256-lane groups per CU, 8 rounds
    { FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_cross_power<real_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const cplx_t*)a, (const cplx_t*)b,
                       (cplx_t*)out, geom(p), scale); }
    FB_LAUNCH_CHECK("k_cross_power");
    return FB_OK;
}
// out_dev[nv][nbins] (nv = nl, or 2 with geom: cells, sum |s|); edges_dev[nbins + 1] on the device, elast = its last value
int FBI(sep_bin)(fb_plan* p, const void* real, const double* edges_dev, double elast, int nbins, int nl, int geom_only,
                 double* out_dev, hipStream_t s) {
    SepGeom sg;
    sg.edges = edges_dev; sg.nbins = nbins; sg.nl = nl; sg.N = p->N;
    for (int a = 0; a < 3; ++a) {
        sg.h[a] = p->L[a] / (double)p->N;
        // |s| >= |m_a| L_a / N: no cell with |m_a| > elast N / L_a reaches a bin (one more for rounding)
        const double q = std::floor(elast * (double)p->N / p->L[a]) + 1.0;
        sg.M[a] = q >= (double)(p->N / 2) ? p->N / 2 : (int)q;
    }
    const int nv = geom_only ? 2 : nl;
    const size_t lds = (size_t)(nbins + 1) * 8 + (size_t)FB_SEP_WAVES * nv * nbins * 8;
    const long long rows = (long long)(sg.M[0] + 1) * (sg.M[1] + 1);
    long long blocks = (rows + FB_SEP_WAVES - 1) / FB_SEP_WAVES;
    if (blocks > p->prow) blocks = p->prow;
    if (blocks < 1) blocks = 1;
    FB_TRY(p->sep_partials.ensure((size_t)blocks * nv * nbins * sizeof(double)));
    if (lds > 65536) {             // more than 2 x 256 bins x 3 multipoles: up to 106 KiB of the CU's 160 KiB (nbins <= 1024)
        FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sep_bin<real_t, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sep_bin<real_t, false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    { FbProfScope _ps(p, FBK_BIN, s);
    if (geom_only)
        hipLaunchKernelGGL((k_sep_bin<real_t, true>), dim3((unsigned)blocks), dim3(64 * FB_SEP_WAVES), lds, s, (const real_t*)real,
                           p->sep_partials, sg);
    else
        hipLaunchKernelGGL((k_sep_bin<real_t, false>), dim3((unsigned)blocks), dim3(64 * FB_SEP_WAVES), lds, s, (const real_t*)real,
                           p->sep_partials, sg); }
    FB_LAUNCH_CHECK("k_sep_bin");
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_bin_finish<>, dim3(nv * nbins), dim3(256), 0, s, p->sep_partials, (int)blocks, nv * nbins, out_dev); }
    FB_LAUNCH_CHECK("k_bin_finish");
    return FB_OK;
}

#ifdef FB_DEFINE_COMMON
// precision-independent: number of full-grid modes per bin
int fbi_bin_count(fb_plan* p, hipStream_t s) {
    FB_HIP(hipMemsetAsync(p->counts, 0, FB_MAX_BINS * sizeof(unsigned long long), s));
    const size_t lds = (size_t)p->nbins * (8 + 8 + 4);
    long long rows = (long long)p->N * p->N;
    int blocks = rows > 1024 ? 1024 : (int)rows;
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_bin_count, dim3(blocks), dim3(256), lds, s, p->counts, geom(p), bin_geom(p)); }
    FB_LAUNCH_CHECK("k_bin_count");
    std::vector<unsigned long long> h(FB_MAX_BINS);
    FB_TRY(fb_read_back(h.data(), p->counts, FB_MAX_BINS * sizeof(unsigned long long), s));
    for (int q = 0; q < FB_MAX_BINS; ++q) p->counts_host[q] = (double)h[(size_t)q];
    return FB_OK;
}
#endif

// ---- foreground maps / cube, radiometer noise (kernels: fb_field_kernels.h, last section) ---------------------
int FBI(sky_colour_map)(fb_plan* p, const void* amp2d, const void* re, const void* im, uint64_t seed, void* out,
                        hipStream_t s) {
    const int n2 = p->N * p->N;
    hipLaunchKernelGGL((k_sky_colour_map<real_t>), dim3((n2 + 255) / 256), dim3(256), 0, s, (const real_t*)amp2d,
                       (const real_t*)re, (const real_t*)im, (cplx_t*)out, n2, rng_key(seed, 0));
    FB_LAUNCH_CHECK("k_sky_colour_map");
    return FB_OK;
}
int FBI(sky_real_plus)(fb_plan* p, const void* in, void* out, double add, hipStream_t s) {
    const int n2 = p->N * p->N;
    hipLaunchKernelGGL((k_sky_real_plus<real_t>), dim3((n2 + 255) / 256), dim3(256), 0, s, (const cplx_t*)in,
                       (real_t*)out, n2, (real_t)add);
    FB_LAUNCH_CHECK("k_sky_real_plus");
    return FB_OK;
}
int FBI(sky_normal_map)(fb_plan* p, const void* unit, uint64_t seed, double mean, double std, void* out, hipStream_t s) {
    const int n2 = p->N * p->N;
    RngKey k = rng_key(seed, 0);
    hipLaunchKernelGGL((k_sky_normal_map<real_t>), dim3((n2 + 255) / 256), dim3(256), 0, s, (const real_t*)unit,
                       (real_t*)out, n2, mean, std, k);
    FB_LAUNCH_CHECK("k_sky_normal_map");
    return FB_OK;
}
int FBI(sky_gaussian)(fb_plan* p, void* map, void* tmp, const double* weights, int radius, hipStream_t s) {
    if (radius < 0 || 2 * radius + 1 > FB_SCRATCH) { fb_set_error("smoothing kernel too wide"); return FB_ERR_INVALID; }
    const int N = p->N, n2 = N * N;
    FB_HIP(hipMemcpyAsync(p->scratch, weights, (size_t)(2 * radius + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL((k_sky_gauss_axis<real_t>), dim3((n2 + 255) / 256), dim3(256), 0, s, (const real_t*)map,
                       (real_t*)tmp, p->scratch, radius, N, 0);
    hipLaunchKernelGGL((k_sky_gauss_axis<real_t>), dim3((n2 + 255) / 256), dim3(256), 0, s, (const real_t*)tmp,
                       (real_t*)map, p->scratch, radius, N, 1);
    FB_LAUNCH_CHECK("k_sky_gauss_axis");
    return FB_OK;
}
int FBI(sky_fg_cube)(fb_plan* p, const void* amps, const void* alpha, double alpha_scalar, const double* ratio,
                     void* out, hipStream_t s) {
    const int N = p->N;
    if (2 * N > FB_SCRATCH) { fb_set_error("grid too large for the frequency table"); return FB_ERR_UNSUPPORTED; }
    std::vector<double> tab((size_t)2 * N);                    // ratio, then log2(ratio)
    for (int z = 0; z < N; ++z) { tab[z] = ratio[z]; tab[N + z] = std::log2(ratio[z]); }
    FB_HIP(hipMemcpyAsync(p->scratch, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    FB_HIP(hipStreamSynchronize(s));                           // `tab` is a local
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_sky_fg_cube<real_t>), dim3((unsigned)((long long)N * N)), dim3(N >= 256 ? 256 : 64), 0, s,
                       (const real_t*)amps, (const real_t*)alpha, alpha_scalar, p->scratch, (real_t*)out, N); }
    FB_LAUNCH_CHECK("k_sky_fg_cube");
    return FB_OK;
}
int FBI(sky_noise_cube)(fb_plan* p, const double* sigma, const void* unit, uint64_t seed, void* out, hipStream_t s) {
    const int N = p->N;
    FB_HIP(hipMemcpyAsync(p->scratch, sigma, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
    const long long n4 = (long long)N * N * N / 4;
    RngKey k = rng_key(seed, 0);
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_sky_noise_cube<real_t>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                       (const real_t*)unit, p->scratch, (real_t*)out, n4, N, k); }
    FB_LAUNCH_CHECK("k_sky_noise_cube");
    return FB_OK;
}

int FBI(real_axpby)(fb_plan* p, const void* x, const void* y, void* out, double a, double b, double c, int mul,
                    hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    const int nb = reduce_blocks(n);
    FbProfScope _ps(p, FBK_REALOP, s);
    if (mul) hipLaunchKernelGGL((k_mul_real<real_t>), dim3(nb), dim3(256), 0, s, (const real_t*)x, (const real_t*)y,
                                (real_t*)out, n);
    else hipLaunchKernelGGL((k_axpby<real_t>), dim3(nb), dim3(256), 0, s, (const real_t*)x, (const real_t*)y,
                            (real_t*)out, n, (real_t)a, (real_t)b, (real_t)c);
    FB_LAUNCH_CHECK("k_axpby");
    return FB_OK;
}

// ---- PCA foreground cleaning (kernels: fb_field_kernels.h, last section) -----------------------------------------
// mean_dev[N] (device, fp64) = mean over the N^2 pixels of every channel (filters.py:142)
int FBI(channel_means)(fb_plan* p, const void* cube, double* mean_dev, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    const int nb = 512 < npix ? 512 : (int)npix;
    FB_TRY(p->work.ensure((size_t)nb * N * sizeof(double)));
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_channel_sums<real_t>), dim3(nb), dim3(256), 0, s, (const real_t*)cube, p->work.as<double>(),
                       npix, N);
    hipLaunchKernelGGL(k_channel_means, dim3((N + 63) / 64), dim3(64, 4), 0, s, p->work.as<const double>(), nb, N,
                       1.0 / (double)npix, mean_dev);
    FB_LAUNCH_CHECK("k_channel_means");
    return FB_OK;
}

// cov_dev[N][N] (device, fp64) = np.cov of the mean-subtracted channels (filters.py:157-158)
int FBI(channel_cov)(fb_plan* p, const void* cube, const double* mean_dev, double* cov_dev, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    const FbCovPlan c = fb_channel_cov_plan(N, p->num_cu);       // block shape and pixel slices: fb_plan.h
    const int MA = c.MA, bs = 16 * MA, nbs = c.nbs, slices = c.slices;
    FB_TRY(p->work.ensure((size_t)slices * N * N * sizeof(double)));
    { FbProfScope _ps(p, FBK_PCA, s);
    const dim3 grid(c.npairs, slices);
    if (MA == 4) hipLaunchKernelGGL((k_channel_cov<real_t, 4>), grid, dim3(64), 0, s, (const real_t*)cube, mean_dev,
                                    p->work.as<double>(), npix, c.rows, N, nbs);
    else if (MA == 2) hipLaunchKernelGGL((k_channel_cov<real_t, 2>), grid, dim3(64), 0, s, (const real_t*)cube, mean_dev,
                                         p->work.as<double>(), npix, c.rows, N, nbs);
    else if (!c.edge) hipLaunchKernelGGL((k_channel_cov<real_t, 1>), grid, dim3(64), 0, s, (const real_t*)cube, mean_dev,
                                         p->work.as<double>(), npix, c.rows, N, nbs);
    else hipLaunchKernelGGL((k_channel_cov<real_t, 1, true>), grid, dim3(64), 0, s, (const real_t*)cube, mean_dev,
                            p->work.as<double>(), npix, c.rows, N, nbs); }
    FB_LAUNCH_CHECK("k_channel_cov");
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_cov_finish, dim3((N + 63) / 64, N), dim3(64), 0, s, p->work.as<const double>(), slices, N, bs,
                       1.0 / (double)(npix - 1), cov_dev); }
    FB_LAUNCH_CHECK("k_cov_finish");
    return FB_OK;
}

// out = cube - mean - U U^T (cube - mean) per pixel; U_dev[N][nm] fp64; amps_dev[nm][N^2] or null
int FBI(pca_clean)(fb_plan* p, const void* cube, const double* mean_dev, const double* U_dev, int nm, void* out,
                   double* amps_dev, hipStream_t s) {
    const int N = p->N;
    const long long npix = (long long)N * N;
    if (nm < 0 || nm > N) { fb_set_error("number of modes out of range"); return FB_ERR_INVALID; }
    const unsigned grid = (unsigned)((npix + 3) / 4);
    FbProfScope _ps(p, FBK_PCA, s);
#define FB_PCA_CASE(C_)                                                                                          \
    hipLaunchKernelGGL((k_pca_clean<real_t, C_>), dim3(grid), dim3(256), 0, s, (const real_t*)cube, mean_dev, U_dev,   \
                       nm, (real_t*)out, amps_dev, npix, N)
    int cpl = 1;                                   // channels per lane: the power of two that covers N / 64
    while (64 * cpl < N) cpl *= 2;
    switch (cpl) {
        case 1: FB_PCA_CASE(1); break;
        case 2: FB_PCA_CASE(2); break;
        case 4: FB_PCA_CASE(4); break;
        case 8: FB_PCA_CASE(8); break;
        case 16: FB_PCA_CASE(16); break;
        case 32: FB_PCA_CASE(32); break;
        default: fb_set_error("unsupported grid size"); return FB_ERR_UNSUPPORTED;
    }
#undef FB_PCA_CASE
    FB_LAUNCH_CHECK("k_pca_clean");
    return FB_OK;
}

int FBI(real_to_complex)(fb_plan* p, const void* in, void* out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    FbProfScope _ps(p, FBK_LAYOUT, s);
    hipLaunchKernelGGL((k_real_to_complex<real_t>), dim3(reduce_blocks(n)), dim3(256), 0, s, (const real_t*)in, (cplx_t*)out, n);
    FB_LAUNCH_CHECK("k_real_to_complex");
    return FB_OK;
}
int FBI(mask_xy)(fb_plan* p, void* cube, const void* mask2d, hipStream_t s) {
    const int N = p->N;
    FbProfScope _ps(p, FBK_FILTER, s);
    hipLaunchKernelGGL((k_mask_xy<real_t>), dim3((unsigned)((long long)N * N)), dim3(N >= 256 ? 256 : 64), 0, s,
                       (cplx_t*)cube, (const real_t*)mask2d, N);
    FB_LAUNCH_CHECK("k_mask_xy");
    return FB_OK;
}
