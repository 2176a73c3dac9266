// Internal plan object behind the opaque `fb_plan*` of include/fastbox_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fb_keyed_cache.h"
#include <string>
#include <vector>

#define FB_OK 0
#define FB_ERR_INVALID -1
#define FB_ERR_HIP -2
#define FB_ERR_UNSUPPORTED -3
#define FB_ERR_NOMEM -4
#define FB_ERR_STATE -5
#define FB_ERR_RCCL -6

void fb_set_error(const std::string& msg);
int fb_hip_check(hipError_t e, const char* what);
#define FB_HIP(x) do { int _r = fb_hip_check((x), #x); if (_r) return _r; } while (0)
#define FB_TRY(x) do { const int _r = (x); if (_r) return _r; } while (0)        // x: a call that returns an FB_* status
#define FB_LAUNCH_CHECK(name) do { int _r = fb_hip_check(hipGetLastError(), name); if (_r) return _r; } while (0)

// Device memory owned by the plan (or by an entry of one of its caches): freed by the destructor, so whoever destroys it makes
// the plan's device current first (fb_plan_destroy; every entry point does).  Grow-only: ensure(bytes) keeps storage that is
// large enough and otherwise frees it before allocating anew -- the contents are lost, and a failed allocation (FB_ERR_NOMEM)
// leaves the buffer empty.  T is what the buffer converts to; as<U>() reads it as another type (the tables in plan precision).
template <typename T = void> struct FbBuf {
    T* ptr = nullptr;
    size_t cap = 0;              // bytes
    FbBuf() = default;
    FbBuf(FbBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    FbBuf(const FbBuf&) = delete;
    FbBuf& operator=(const FbBuf&) = delete;
    ~FbBuf() { if (ptr) (void)hipFree(ptr); }
    operator T*() const { return ptr; }
    template <typename U> U* as() const { return static_cast<U*>(static_cast<void*>(ptr)); }
    int ensure(size_t need) { return cap >= need ? FB_OK : grow(need); }
    int reset() {                // back to empty
        T* q = ptr;
        ptr = nullptr; cap = 0;
        if (q) FB_HIP(hipFree(q));
        return FB_OK;
    }
private:
    __attribute__((noinline)) int grow(size_t need) {       // the rare path stays out of line, so that ensure() inlines to its comparison
        FB_TRY(reset());
        FB_HIP(hipMalloc(reinterpret_cast<void**>(&ptr), need));
        cap = need;
        return FB_OK;
    }
};

struct fb_comm;                  // fb_comm.inc: RCCL communicator + its stream and events (fb_comm_create)

// One k_perp edge set's transverse rows (m_x, m_y), as i N + j, sorted by bin (ascending inside a bin): what both estimators
// of fb_cyl.hip gather through.  A row lies in bin np.digitize(k_perp, edges) - 1 with k_perp = sqrt(k_x k_x + k_y k_y) formed
// on the host exactly as numpy forms it; rows outside [edges[0], edges[nb]) are not listed.  The plan's cache keys an entry by
// (edges[nb + 1], skip0); skip0: the row m_perp = 0 is left out.
struct fb_cyl_rows {
    int nb = 0;
    FbBuf<int> rows_dev;                 // [off[nb]]
    std::vector<int> off;                // [nb + 1] first row of each bin
    std::vector<double> sumk;            // [nb] sum of k_perp over the bin's rows
    bool has0 = false;                   // the row m_perp = 0 is listed (in bin 0: k_perp = 0)
};

struct fb_plan {
    fb_comm* comm = nullptr;     // one box over several GPUs: this rank's communicator, or null
    int N = 0;
    int generic = 0;         // 1: N is not a power of two (even, factors 2, 3, 5, <= 1024): the plain passes of fb_fft_generic.h, no fused entry points
    int prec = 4;            // bytes per real: 4 (float) or 8 (double)
    double L[3] = {0, 0, 0};
    int device = 0;
    int debug_no_mem = 0;    // tuning aid (fb_debug_strided_pass mode >= 10)
    int pass_schedule[3] = {-1, -1, -1};   // per strided-pass class (plain, generator, binning): 0 one workgroup per tile,
                                           // 1 resident workgroups walking the tiles, -1 by grid size (fb_set_pass_schedule)
    int wide_rows = -1;      // strided passes at N = 2048, single precision: bit mask of the pass classes (1 plain, 2 generator, 4 binning)
                             // that run in 128-byte rows; -1: the library's choice (fb_set_tile_rows; FB_WIDE_ROWS=<mask> overrides it)
    int plane_batch = -1;    // x-planes per batch of the y/z passes: -1 sized to the Infinity Cache, 0 whole box (fb_set_plane_batching)
    int plane_streams = 0;   // 1 | 2 streams for alternate batches; 0: by grid size
    double exp_shift = 0.0;  // fused log-normal transforms use exp(x - exp_shift) (fb_set_exp_shift)
    int num_cu = 256;        // compute units of the device (persistent-grid sizing)
    int NZV = 0;             // stored k_z modes of a half spectrum: N/2+1
    int NZP = 0;             // row pitch of a half spectrum (complex elements)
    int NR = 0;              // stored rows per x-plane of a half spectrum (N + 1: see KGeom::NR)
    int cubic = 0;           // Lx == Ly == Lz (integer shells usable)

    FbBuf<> tw;              // forward twiddles W_N^j, j < N, in plan precision
    FbBuf<double> axis2;     // [3][N] (m_i / L_a)^2 exactly as numpy computes it (box.py:125-127)
    FbBuf<double> kpar;      // [N]  2 pi m / Lz
    FbBuf<double> ksc;       // [3][N] m_i * (2 pi / L_a)  (velocity numerators, box.py:254-256)
    FbBuf<double> zgrid;     // [N]  self.z

    // sqrt(P(k) boxfactor) lookup (box.py:161-176)
    FbBuf<> amp_shell;           // [nshell] plan precision, index n^2 = i^2+j^2+l^2 (cubic only)
    int64_t nshell = 0;
    const void* amp_dense = nullptr;  // caller-owned [N][N][NZP]
    // The shared work buffer of the cleaning, in-painting, bispectrum, line-of-sight-fit and channel mean / covariance entry
    // points.  The rule that lets them share it: its contents are undefined on entry to every entry point, and no entry point
    // keeps a pointer into it after it returns -- each lays it out anew (its ensure() may move it).  Whatever has to outlive a
    // call gets a buffer of its own.
    FbBuf<> work;
    FbBuf<double> eig_work;      // [4 n^2 + 2] of fb_leading_eigenvectors: its input may be a covariance computed through `work`
    FbBuf<double> kperp_tab;     // [N][N] 2 pi sqrt((m_x/L_x)^2 + (m_y/L_y)^2), box.py:374
    int amp_sym_only = 0;        // amp_sym was given directly (any box shape); no shell table behind it
    FbBuf<> amp_sym;             // [N/2+1][N/2+1][NZP] plan precision: amp_shell spread over (|m_x|, |m_y|, k_z)

    // P(k) binning (box.py:745-764)
    FbBuf<double> bins;          // [nbins] edges
    int nbins = 0;
    FbBuf<int> thr;              // [FB_MAX_BINS] shell thresholds (cubic boxes)
    int use_thr = 0;             // 0: decide every mode with the exact fp64 |k|
    int namb = 0;
    int amb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    FbBuf<unsigned long long> counts;      // [FB_MAX_BINS] device
    double counts_host[256];
    FbBuf<double> partials;      // [prow][3*FB_MAX_BINS] per-workgroup partial sums
    int prow = 0;
    FbBuf<double> scratch;       // small reduction scratch [FB_SCRATCH]
    FbBuf<double> bin_partials;       // fused binning: [workgroups][2*nbins] (grown on demand)
    long long bin_rows = 0;
    long long bin_rows_main = 0;      // of which the fused binning pass itself wrote (the rest: k_bin_packed_plane)
    long long bin_append_cols = 0;    // > 0: binning launches append their columns to a shared table of this many (k_z chunks)
    FbBuf<> plane_buf;                // packed work spectra: the shared plane column after the last forward pass, [N][N] complex
    FbBuf<double> exp_partials;       // r2c with exp(): [workgroups] (grown on demand)
    long long exp_rows = 0;
    long long exp_base = 0;           // block offset of the plane batch being launched (fb_fft_launch.inc yz_passes)

    // correlation function (fb_bin_separation): edges on the device, and the data-independent sums (cells, sum |s|) per
    // bin set already computed -- key [edges...], value [cells..., sum |s|...]
    FbBuf<double> sep_edges;          // [FB_MAX_SEP_BINS + 1] (allocated on first use)
    FbKeyedCache<std::vector<double>, 16> sep_geom;
    FbBuf<double> sep_partials;       // [nv nbins][workgroups] of k_sep_bin (grown on demand: up to 3 x 1024 values per workgroup)

    // power spectrum in (k, mu) bins (fb_power.hip): the bin table on the device, per-workgroup partials, and the
    // data-independent sums (modes, sum |k|, sum mu per cell) per (edges, nmu) already computed -- key [edges..., nmu], value
    // [modes..., sum |k|..., sum mu...]
    FbBuf<double> pk_tab;             // [FB_PK_MAX_K + FB_PK_MAX_MU + 2] (allocated on first use)
    FbBuf<double> pk_partials;        // [values][workgroups] of k_pk_bin (grown on demand)
    FbKeyedCache<std::vector<double>, 16> pk_geom;

    // cylindrical power and multi-frequency angular power (fb_cyl.hip): the transverse rows sorted by k_perp bin per edge set
    // already seen, the chunk / fold tables of the call in flight, the partials
    FbKeyedCache<fb_cyl_rows, 8> cyl_rows;
    FbBuf<int> cyl_idx;               // [3 chunks][nb + 1 chunk offsets][2 npar m_z ranges] (grown on demand)
    FbBuf<double> cyl_tab;            // [nb] Lx Ly / (N^4 modes_b) of fb_transverse_gram (grown on demand)
    FbBuf<double> cyl_partials;       // [chunks][N/2 + 1] of k_cyl_rows (grown on demand)

    // halo tracers (fb_halo.hip): reduction partials, the catalogue's (count, block) tables, the painting accumulators
    FbBuf<> halo_small;               // [FB_HALO_SMALL] bytes (allocated on first use)
    FbBuf<> halo_work;                // grown on demand
    FbBuf<> halo_acc;                 // grown on demand

    // void finding (fb_voids.hip): flags and reduction partials, and the per-label / per-tile work tables
    FbBuf<> void_small;               // [FB_VOID_SMALL] bytes (allocated on first use)
    FbBuf<> void_work;                // grown on demand

    // second stream for alternate plane batches of the y/z passes (created on first use)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // per-kernel HIP-event timing (fb_profile_start / fb_profile_stop)
    bool prof_on = false;
    unsigned prof_mask = 0xFFFFFFFFu;   // kernel classes to bracket (bit = FBK_* index)
    int prof_stride = 1;                // bracket every prof_stride-th selected launch (fb_profile_sample)
    long long prof_seen = 0;            // selected launches since fb_profile_start
    std::vector<hipEvent_t> prof_ev;   // pairs
    std::vector<int> prof_cat;
    size_t prof_used = 0;
};

// kernel classes reported by fb_profile_stop (keep in sync with FB_PROF_* in fastbox_hip.h)
enum { FBK_FFT_STRIDED = 0, FBK_FFT_CONTIG, FBK_COLOUR, FBK_BIN, FBK_FILTER, FBK_VELPOT, FBK_REALOP, FBK_RSD,
       FBK_LAYOUT, FBK_FFT_GEN, FBK_FFT_BIN, FBK_PCA, FBK_NCAT };

// RAII: records an event pair around one launch while profiling is on
struct FbProfScope {
    fb_plan* p; hipStream_t s; size_t slot; bool on;
    FbProfScope(fb_plan* plan, int cat, hipStream_t stream)
        : p(plan), s(stream), slot(0), on(plan->prof_on && ((plan->prof_mask >> cat) & 1u)) {
        if (!on) return;
        if ((p->prof_seen++ % p->prof_stride) != 0) { on = false; return; }
        if (p->prof_used + 2 > p->prof_ev.size()) {
            for (int q = 0; q < 64; ++q) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
                                           p->prof_ev.push_back(e); }
        }
        slot = p->prof_used; p->prof_used += 2;
        p->prof_cat.resize(p->prof_used / 2); p->prof_cat[slot / 2] = cat;
        (void)hipEventRecord(p->prof_ev[slot], s);
    }
    ~FbProfScope() { if (on) (void)hipEventRecord(p->prof_ev[slot + 1], s); }
};

#define FB_MAX_BINS 256
#define FB_MAX_SEP_BINS 1024     // separation bins of fb_bin_separation: the default edges of a 2048^3 box (dr = L/N, rmax = L/2)
#define FB_PK_MAX_K 1024         // k bins of fb_bin_power_kmu: the default edges of a 2048^3 box (dk = 2 pi / L up to Nyquist)
#define FB_PK_MAX_MU 128         // mu bins
#define FB_PK_MAX_VALUES 5120    // nk nmu (lmax / 2 + 1): one wave's LDS row of 40 KiB (1024 k bins x 5 mu bins)
#define FB_SCRATCH 8192

// ---- per-precision launchers (fb_fft_launch.inc, fb_field_launch.inc) ------------
#define FB_DECL(sfx) \
    int fbi_fft_c2c_##sfx(fb_plan* p, void* data, int sign, double scale, hipStream_t s); \
    int fbi_fft_r2c_##sfx(fb_plan* p, const void* real_in, void* half_out, int pre_exp, hipStream_t s); \
    int fbi_fft_c2r_##sfx(fb_plan* p, void* half_inout, void* real_out, double scale, hipStream_t s); \
    int fbi_set_amp_shells_##sfx(fb_plan* p, const double* amp, int64_t n); \
    int fbi_set_amp_sym_##sfx(fb_plan* p, const double* amp, int64_t n); \
    int fbi_colour_noise_##sfx(fb_plan* p, const void* re, const void* im, void* out, hipStream_t s); \
    int fbi_colour_device_##sfx(fb_plan* p, uint64_t seed, uint64_t real, void* out, hipStream_t s); \
    int fbi_power_filtered_##sfx(fb_plan* p, const void* real_in, void* filtered_half, int kind, const double* prm, \
                                 const void* table, double* results, int inverse_x, hipStream_t s); \
    int fbi_fft_c2r_yz_##sfx(fb_plan* p, void* half_inout, void* real_out, double scale, hipStream_t s); \
    int fbi_realise_velocity_begin_##sfx(fb_plan* p, uint64_t seed, uint64_t real, int comp, double fac, void* work_half, \
                                         hipStream_t s); \
    int fbi_power_redshift_space_##sfx(fb_plan* p, void* work_d, void* work_v, void* real_d_out, void* out_half, double scale, \
                                       double Hz, double sigma_nl, uint64_t seed, int nearest, int kind, const double* prm, \
                                       const void* table, double* results, int inverse_x, hipStream_t s); \
    int fbi_slab_forward_packed_##sfx(fb_plan* p, const void* real_local, void* half_local, void* xbuf, int nxl, \
                                      int nparts, int pre_exp, double* expsum, hipStream_t s); \
    int fbi_slab_inverse_packed_##sfx(fb_plan* p, const void* xbuf, void* half_local, void* real_local, int nxl, \
                                      int nparts, double scale, hipStream_t s); \
    int fbi_slab_turnaround_##sfx(fb_plan* p, const void* recvbuf, void* half_local, void* real_local, void* sendbuf, \
                                  int nxl, int nparts, double scale, int pre_exp, double* expsum, hipStream_t s); \
    int fbi_channel_means_##sfx(fb_plan* p, const void* cube, double* mean_dev, hipStream_t s); \
    int fbi_channel_cov_##sfx(fb_plan* p, const void* cube, const double* mean_dev, double* cov_dev, hipStream_t s); \
    int fbi_pca_clean_##sfx(fb_plan* p, const void* cube, const double* mean_dev, const double* U_dev, int nm, \
                            void* out, double* amps_dev, hipStream_t s); \
    int fbi_real_axpby_##sfx(fb_plan* p, const void* x, const void* y, void* out, double a, double b, double c, \
                             int mul, hipStream_t s); \
    int fbi_fft_axes01_##sfx(fb_plan* p, void* data, int sign, double scale, hipStream_t s); \
    int fbi_beam_convolve_##sfx(fb_plan* p, const void* field, const void* beam, void* work_a, void* work_b, void* out, \
                                int flags, hipStream_t s); \
    int fbi_real_to_complex_##sfx(fb_plan* p, const void* in, void* out, hipStream_t s); \
    int fbi_mask_xy_##sfx(fb_plan* p, void* cube, const void* mask2d, hipStream_t s); \
    int fbi_fft2d_c2c_##sfx(fb_plan* p, void* data, int sign, double scale, hipStream_t s); \
    int fbi_sky_colour_map_##sfx(fb_plan* p, const void* amp2d, const void* re, const void* im, uint64_t seed, \
                                 void* out, hipStream_t s); \
    int fbi_sky_real_plus_##sfx(fb_plan* p, const void* in, void* out, double add, hipStream_t s); \
    int fbi_sky_normal_map_##sfx(fb_plan* p, const void* unit, uint64_t seed, double mean, double std, void* out, \
                                 hipStream_t s); \
    int fbi_sky_gaussian_##sfx(fb_plan* p, void* map, void* tmp, const double* weights, int radius, hipStream_t s); \
    int fbi_sky_fg_cube_##sfx(fb_plan* p, const void* amps, const void* alpha, double alpha_scalar, \
                              const double* ratio, void* out, hipStream_t s); \
    int fbi_sky_noise_cube_##sfx(fb_plan* p, const double* sigma, const void* unit, uint64_t seed, void* out, \
                                 hipStream_t s); \
    int fbi_cross_power_##sfx(fb_plan* p, const void* a, const void* b, void* out, double scale, hipStream_t s); \
    int fbi_sep_bin_##sfx(fb_plan* p, const void* real, const double* edges_dev, double elast, int nbins, int nl, \
                          int geom_only, double* out_dev, hipStream_t s); \
    int fbi_bin_power_##sfx(fb_plan* p, const void* spec, int layout, int filter_kind, const double* prm, \
                            const void* table, double* sums_dev, hipStream_t s); \
    int fbi_apply_filter_##sfx(fb_plan* p, const void* in, void* out, int layout, int kind, const double* prm, \
                               const void* table, hipStream_t s); \
    int fbi_velocity_##sfx(fb_plan* p, const void* dk, void* out, int layout, int comp, double fac, hipStream_t s); \
    int fbi_potential_##sfx(fb_plan* p, const void* dk, void* out, int layout, hipStream_t s); \
    int fbi_lognormal_##sfx(fb_plan* p, const void* in, void* out, double* mean_out, hipStream_t s); \
    int fbi_rsd_##sfx(fb_plan* p, const void* d, const void* vz, const void* noise, void* out, double Hz, \
                      double sigma, uint64_t seed, int nearest, hipStream_t s); \
    int fbi_sum_real_##sfx(fb_plan* p, const void* x, int squared, double* out, hipStream_t s); \
    int fbi_max_real_##sfx(fb_plan* p, const void* x, double* out, hipStream_t s); \
    int fbi_sumsq_half_##sfx(fb_plan* p, const void* h, double* out, hipStream_t s); \
    int fbi_expand_half_##sfx(fb_plan* p, const void* h, void* f, hipStream_t s); \
    int fbi_crop_full_##sfx(fb_plan* p, const void* f, void* h, hipStream_t s); \
    int fbi_realise_velocity_fused_##sfx(fb_plan* p, uint64_t seed, uint64_t real, int comp, double fac, \
                                         void* work_half, void* real_out, double scale, hipStream_t s); \
    int fbi_realise_fused_##sfx(fb_plan* p, uint64_t seed, uint64_t real, void* work_half, void* real_out, \
                                double scale, hipStream_t s); \
    int fbi_power_fused_##sfx(fb_plan* p, const void* real_in, void* work_half, int pre_exp, int store, \
                              double* results, hipStream_t s); \
    int fbi_debug_pass_##sfx(fb_plan* p, void* half, int axis, int mode, hipStream_t s); \
    int fbi_realise_begin_##sfx(fb_plan* p, uint64_t seed, uint64_t real, void* work_half, hipStream_t s); \
    int fbi_realise_finish_##sfx(fb_plan* p, void* work_half, void* real_out, double scale, hipStream_t s); \
    int fbi_power_from_pending_##sfx(fb_plan* p, void* work_half, void* real_out, double scale, int pre_exp, \
                                     double* results, hipStream_t s); \
    int fbi_slab_forward_local_##sfx(fb_plan* p, const void* real_local, void* half_local, int nxl, int pre_exp, \
                                     double* expsum, hipStream_t s); \
    int fbi_slab_inverse_local_##sfx(fb_plan* p, void* half_local, void* real_local, int nxl, double scale, hipStream_t s); \
    int fbi_slab_x_pass_##sfx(fb_plan* p, void* kslab, int nyl, int sign, hipStream_t s); \
    int fbi_slab_x_generate_##sfx(fb_plan* p, void* kslab, int nyl, int ky0, uint64_t seed, uint64_t real, hipStream_t s); \
    int fbi_slab_x_bin_##sfx(fb_plan* p, void* kslab, int nyl, int ky0, double* results, hipStream_t s); \
    int fbi_slab_tile_cols_##sfx(const fb_plan* p); \
    int fbi_slab_x_generate_chunk_##sfx(fb_plan* p, void* kchunk, int nyl, int ky0, uint64_t seed, uint64_t real, int tile0, \
                                        int ntile, hipStream_t s); \
    int fbi_slab_y_inverse_chunk_##sfx(fb_plan* p, const void* recv_chunk, void* half_local, int nxl, int nparts, int tile0, \
                                       int ntile, hipStream_t s); \
    int fbi_slab_y_forward_chunk_##sfx(fb_plan* p, const void* half_local, void* send_chunk, int nxl, int nparts, int tile0, \
                                       int ntile, hipStream_t s); \
    int fbi_slab_z_pass_##sfx(fb_plan* p, void* half_local, void* real_local, int nxl, int which, double scale, int pre_exp, \
                              double* expsum, hipStream_t s); \
    int fbi_slab_x_bin_chunk_##sfx(fb_plan* p, void* kchunk, int nyl, int ky0, int tile0, int ntile, int first, int last, \
                                   double* results, hipStream_t s);
FB_DECL(f32)
FB_DECL(f64)
// The launch plan of k_channel_cov (fbi_channel_cov, fb_channel_covariance_plan): blocks of 16 MA channels -- the largest of
// 64, 32, 16 that divides N; a grid whose size is no multiple of 16 (18, 30, 50, ...) takes 16-channel blocks with a masked last
// one -- and the split of the N^2 pixels into `slices` runs of `rows` pixels: about 8 waves per CU (two rounds of one per SIMD)
// over all block pairs, at least 64 pixels each, `rows` a multiple of 4 (one matrix instruction takes 4 pixels).  Every slice
// is non-empty and they tile [0, N^2): slice q is [q rows, min((q + 1) rows, N^2)), slices = ceil(N^2 / rows).
struct FbCovPlan { int MA, nbs, npairs, slices; bool edge; long long rows; };
inline FbCovPlan fb_channel_cov_plan(int N, int num_cu) {
    FbCovPlan c;
    const long long npix = (long long)N * N;
    c.MA = N % 64 == 0 ? 4 : (N % 32 == 0 ? 2 : 1);
    c.edge = N % 16 != 0;
    const int bs = 16 * c.MA;
    c.nbs = (N + bs - 1) / bs;
    c.npairs = c.nbs * (c.nbs + 1) / 2;
    long long want = (8LL * num_cu + c.npairs - 1) / c.npairs;
    if (want > npix / 64) want = npix / 64;
    if (want < 1) want = 1;
    c.rows = ((npix + want - 1) / want + 3) & ~3LL;
    c.slices = (int)((npix + c.rows - 1) / c.rows);        // <= want: rounding `rows` up can only empty the last of them
    return c;
}
// The pixel partitions of k_nmf_sweep (nmf_sweep, fb_nmf_sweep_plan) and of k_ica_step (fb_ica_step, fb_ica_step_plan):
// workgroup q takes the pixels [q per, min((q + 1) per, N^2)).  Trailing workgroups whose share starts at or past N^2 are empty:
// they read no pixel and write a partial of zeros.  The sweep walks four pixels at a time (one per wave): two workgroups per CU,
// `per` a multiple of 4.  The ICA step: about 64 pixels per workgroup, at most 1024 workgroups (FB_CLEAN_RED_BLOCKS).
struct FbPixelSplit { int workgroups; long long per; };
inline FbPixelSplit fb_nmf_sweep_split(int N, int num_cu) {
    const long long npix = (long long)N * N;
    long long nb = (npix + 3) / 4;
    if (nb > 2LL * num_cu) nb = 2LL * num_cu;
    return FbPixelSplit{(int)nb, ((npix + nb - 1) / nb + 3) & ~3LL};
}
inline FbPixelSplit fb_ica_step_split(int N) {
    const long long npix = (long long)N * N;
    long long nb = (npix + 63) / 64;
    if (nb > 1024) nb = 1024;
    return FbPixelSplit{(int)nb, (npix + nb - 1) / nb};
}
int fbi_bin_count(fb_plan* p, hipStream_t s);
int fbi_slab_permute(fb_plan* p, const void* in, void* out, int nxl, int nparts, int pack, hipStream_t s);
