// Host launchers for one precision.  Included by fb_fft_f32.hip / fb_fft_f64.hip
// with FB_REAL defined to float / double and FB_SUFFIX to f32 / f64.
#include <cstdlib>
#include <cstring>
#include "fb_plan.h"
#include "fb_fft_kernels.h"
#include "fb_fft_generic.h"

namespace {

using namespace fb;
typedef FB_REAL real_t;
typedef cx<real_t> cplx_t;

template <typename K> int set_lds(K kernel, size_t bytes) {
    if (bytes > 65536)
        FB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return FB_OK;
}

KGeom fft_geom(const fb_plan* p) { return KGeom{p->axis2, p->ksc, p->kpar, p->N, p->NZV, p->NZP, p->NR}; }
// which amplitude table the fused generator reads: the k_z-contiguous table when there is one (built from the
// shell table of a cubic box, or given directly for any box shape), else the caller's dense per-mode table
int gen_amplitude(const fb_plan* p, StridedOp<real_t>& op) {
    op.amp.shell = (p->amp_dense || p->amp_sym_only) ? nullptr : p->amp_shell.as<const real_t>();
    op.amp.dense = p->amp_sym_only ? nullptr : reinterpret_cast<const real_t*>(p->amp_dense);
    op.amp.sym = (op.amp.shell || p->amp_sym_only) ? p->amp_sym.as<const real_t>() : nullptr;
    if (!op.amp.shell && !op.amp.dense && !op.amp.sym) { fb_set_error("amplitude table not set (fb_set_amplitude_*)"); return FB_ERR_STATE; }
    return FB_OK;
}

// PERSIST: resident workgroups that walk the tiles (k_fft_strided); 0: one workgroup per tile.  BLK: slab addressing.
template <int N, int MODE, int PERSIST, bool BLK>
int launch_strided_npb(fb_plan* p, const StridedArgs<real_t>& a, int nouter, int sign, StridedOp<real_t>& op,
                       hipStream_t s) {
    constexpr bool SPLIT = strided_split<real_t>(N, MODE, BLK);
    constexpr int E = strided_elems_of<real_t>(N, MODE, BLK), TPL = N / E, TZ = tile_cols_of<real_t>(N, MODE, BLK);
    constexpr int NW = (TZ * TPL + 63) / 64;
    size_t lds = (size_t)N * TZ * (SPLIT ? sizeof(real_t) : sizeof(cplx_t)) + (size_t)N * sizeof(cplx_t);
    if (smode_bins(MODE)) lds += (size_t)NW * 2 * op.nbins * sizeof(double) + (size_t)((op.nbins + 63) & ~63) * sizeof(int);
    StridedArgs<real_t> b = a;
    b.ntx = a.ntx ? a.ntx : (a.ncols + TZ - 1) / TZ;        // (a.ntx given: a range of tile columns, StridedArgs::tile0)
    b.ntiles = b.ntx * nouter;
    b.ntx_shift = -1;
    for (int q = 0; q < 30; ++q) if ((1 << q) == b.ntx) b.ntx_shift = q;
    // one 64-bit base per tile + a 32-bit scalar offset per point, unless a line's last point is too far from its first
    b.wide = ((long long)(E - 1) * TPL * a.stride * (long long)sizeof(cplx_t) >= 0xE0000000LL) ? 1 : 0;
    b.drop_io = p->debug_no_mem;           // tuning aid: same grid and arithmetic, every access out of range
    auto pick = [&]() {
#ifndef FB_CSIGN_FROM
#define FB_CSIGN_FROM (1 << 30)       // tuning: plain passes of lines this long compile the direction in as well (see CSIGN)
#endif
        if constexpr (MODE == SMODE_PLAIN && (strided_row128<real_t>(N, MODE, BLK) || N >= (FB_CSIGN_FROM)))     // one kernel per direction (see CSIGN)
            return sign < 0 ? k_fft_strided<real_t, N, MODE, PERSIST, BLK, -1> : k_fft_strided<real_t, N, MODE, PERSIST, BLK, +1>;
        else return k_fft_strided<real_t, N, MODE, PERSIST, BLK>;
    };
    auto kernel = pick();
    int r = set_lds(kernel, lds);
    if (r) return r;
    int nblk = b.ntiles;
    if (PERSIST) {
        // resident grid: as many workgroups as the chip holds at once (LDS- and thread-limited; asked once per kernel)
        static thread_local int per_cu = 0;
        static thread_local size_t per_cu_lds = 0;      // (the binning pass's LDS grows with the number of bins)
        if (!per_cu || per_cu_lds != lds) {
            int q = 1;
            FB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kernel, TZ * TPL, lds));
            per_cu = q < 1 ? 1 : (q > 4 ? 4 : q);
            per_cu_lds = lds;
        }
        if (per_cu * p->num_cu < nblk) nblk = per_cu * p->num_cu;
    }
    // (a chunk sequence that was never closed -- an exception or a failed collective between two fb_slab_x_bin_chunk calls --
    // must not turn a later whole-spectrum binning launch into an append: only launches over a tile range append)
    if (smode_bins(MODE) && p->bin_append_cols && !a.ntx) p->bin_append_cols = 0;
    if (smode_bins(MODE) && p->bin_append_cols) {
        // one of several launches that share a table of partial sums (the k_z chunks of the slab-decomposed transform):
        // this one's workgroups take the next nblk columns of a table of p->bin_append_cols (allocated by the caller)
        if (p->bin_rows + nblk > p->bin_append_cols) { fb_set_error("binning chunks exceed the partial-sum table"); return FB_ERR_STATE; }
        op.partial = p->bin_partials + p->bin_rows;
        op.partial_stride = p->bin_append_cols;
        p->bin_rows += nblk;
        p->bin_rows_main = p->bin_rows;
    } else if (smode_bins(MODE)) {
        const long long rows = nblk + (a.packed ? N : 0);     // packed: one more column per k_y row (k_bin_packed_plane)
#ifdef FB_STAMPS
        r = p->bin_partials.ensure(((size_t)rows * 2 * op.nbins + (size_t)nblk * 32 + 64) * sizeof(double));
#else
        r = p->bin_partials.ensure((size_t)rows * 2 * op.nbins * sizeof(double));
#endif
        if (r) return r;
        op.partial = p->bin_partials;
        op.partial_stride = rows;
        p->bin_rows = rows;
        p->bin_rows_main = nblk;
    }
    { FbProfScope _ps(p, MODE == SMODE_GEN ? FBK_FFT_GEN : (smode_bins(MODE) ? FBK_FFT_BIN : FBK_FFT_STRIDED), s);
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(TZ * TPL), lds, s, b, sign, op); }
    FB_LAUNCH_CHECK("k_fft_strided");
    return FB_OK;
}
#ifndef FB_WIDE_ROWS_DEFAULT
#define FB_WIDE_ROWS_DEFAULT 1
#endif
template <int N, int MODE, int PERSIST>
int launch_strided_np(fb_plan* p, const StridedArgs<real_t>& a, int nouter, int sign, StridedOp<real_t>& op,
                      hipStream_t s) {
    if constexpr (MODE == SMODE_PLAIN) {
        if (a.blk_in || a.blk_out) return launch_strided_npb<N, MODE, PERSIST, true>(p, a, nouter, sign, op, s);
    }
    if constexpr (MODE == SMODE_GEN && strided_wide<real_t>(N, MODE, false)) {
        // a launch over a range of tile columns (k_z chunks of the slab path): the range is counted in the narrow tiles
        if (a.ntx || a.tile0) return launch_strided_npb<N, MODE, PERSIST, true>(p, a, nouter, sign, op, s);
    }
    if constexpr (strided_row128<real_t>(N, MODE, false)) {
        // 128-byte-row form (N = 2048): a launch over a range of tile columns (the slab path's k_z chunks, counted in the narrow
        // tiles) and a plan set to 64-byte rows (fb_set_tile_rows) keep the narrow tile = the kernels with slab addressing
        // Which classes take the wide form by default: measured on MI355X (tools/pass_bench.py 2048, profiles/r04_pass_bench_2048.txt)
        static const char* env = getenv("FB_WIDE_ROWS");
        const int mask = env ? atoi(env) : (p->wide_rows >= 0 ? p->wide_rows : FB_WIDE_ROWS_DEFAULT);
        const int bit = MODE == SMODE_PLAIN ? 1 : (MODE == SMODE_GEN ? 2 : 4);
        if (!(mask & bit) || a.ntx || a.tile0) return launch_strided_npb<N, MODE, PERSIST, true>(p, a, nouter, sign, op, s);
    }
    return launch_strided_npb<N, MODE, PERSIST, false>(p, a, nouter, sign, op, s);
}

// which form a pass runs in: the plan's schedule per pass class (fb_set_pass_schedule; -1 = by grid size;
// FB_PASS_SCHEDULE = three digits "plain gen bin" overrides it, tuning aid).  Measured on MI355X
// (tools/pass_bench.py, profiles/r03_pass_schedules.txt): the resident form wins where a CU holds ONE workgroup of the
// pass (16 points per thread, N = 2048: x passes -13 %, generator -7 %, binning -11 %; nothing else hides a workgroup's
// load latency there) and loses where it holds two (N <= 1024: two resident workgroups that started together stay in
// step and want the same unit at the same time, and the tile loop's extra scalar state spills; -5 ... -20 %).
template <int N, int MODE>
int launch_strided_n(fb_plan* p, const StridedArgs<real_t>& a, int nouter, int sign, StridedOp<real_t>& op,
                     hipStream_t s) {
    if constexpr (N >= 256 && MODE != SMODE_BINF) {      // (the filtering pass has no registers to spare for the next tile's loads)
        static const char* env = getenv("FB_PASS_SCHEDULE");
        const int cls = MODE == SMODE_GEN ? 1 : (smode_bins(MODE) ? 2 : 0);
        static const bool env_ok = env && strlen(env) == 3 && strspn(env, "01") == 3;       // anything else is ignored, not read as 0
        int sched = env_ok ? env[cls] - '0' : p->pass_schedule[cls];
        if (sched < 0) sched = strided_elems_of<real_t>(N, MODE, MODE == SMODE_GEN && (a.ntx || a.tile0)) > 8 ? 1 : 0;
        if (sched == 1) return launch_strided_np<N, MODE, 1>(p, a, nouter, sign, op, s);
    }
    return launch_strided_np<N, MODE, 0>(p, a, nouter, sign, op, s);
}

template <int MODE>
int launch_strided(fb_plan* p, int N, const StridedArgs<real_t>& a, int nouter, int sign, StridedOp<real_t>& op,
                   hipStream_t s) {
    switch (N) {
        case 16: return launch_strided_n<16, MODE>(p, a, nouter, sign, op, s);
        case 32: return launch_strided_n<32, MODE>(p, a, nouter, sign, op, s);
        case 64: return launch_strided_n<64, MODE>(p, a, nouter, sign, op, s);
        case 128: return launch_strided_n<128, MODE>(p, a, nouter, sign, op, s);
        case 256: return launch_strided_n<256, MODE>(p, a, nouter, sign, op, s);
        case 512: return launch_strided_n<512, MODE>(p, a, nouter, sign, op, s);
        case 1024: return launch_strided_n<1024, MODE>(p, a, nouter, sign, op, s);
        case 2048: return launch_strided_n<2048, MODE>(p, a, nouter, sign, op, s);
    }
    fb_set_error("unsupported grid size (need a power of two, 16..2048)");
    return FB_ERR_UNSUPPORTED;
}
int launch_plain(fb_plan* p, int N, const StridedArgs<real_t>& a, int nouter, int sign, hipStream_t s) {
    StridedOp<real_t> op = {};
    return launch_strided<SMODE_PLAIN>(p, N, a, nouter, sign, op, s);
}

template <int NF, int MODE>
int launch_contig_n(fb_plan* p, ContigArgs<real_t>& a, int sign, hipStream_t s) {
    constexpr int E = elems_per_thread<real_t>(NF), TPL = NF / E, LPW = contig_lines<real_t, NF>();
    constexpr int M = NF * (MODE == ZMODE_C2C ? 1 : 2);
    const size_t lds = (size_t)(LPW * LineLayout<real_t>::padded(NF) + M) * sizeof(cplx_t);
    int r = set_lds(k_fft_contig<real_t, NF, MODE>, lds);
    if (r) return r;
    const long long nblk = (a.nlines + LPW - 1) / LPW;
    a.exp_shift = (real_t)p->exp_shift;
    if ((MODE == ZMODE_R2C || MODE == ZMODE_C2R2C) && a.pre_exp) {     // exp_base: blocks of earlier plane batches
        r = p->exp_partials.ensure((size_t)(p->exp_base + nblk) * sizeof(double));
        if (r) return r;
        a.exp_partial = p->exp_partials + p->exp_base;
        p->exp_rows = p->exp_base + nblk;
    }
    { FbProfScope _ps(p, FBK_FFT_CONTIG, s);
    hipLaunchKernelGGL((k_fft_contig<real_t, NF, MODE>), dim3((unsigned)nblk), dim3(LPW * TPL), lds, s, a, sign); }
    FB_LAUNCH_CHECK("k_fft_contig");
    return FB_OK;
}

template <int MODE>
int launch_contig(fb_plan* p, int NF, ContigArgs<real_t>& a, int sign, hipStream_t s) {
    switch (NF) {
        case 8: return launch_contig_n<8, MODE>(p, a, sign, s);
        case 16: return launch_contig_n<16, MODE>(p, a, sign, s);
        case 32: return launch_contig_n<32, MODE>(p, a, sign, s);
        case 64: return launch_contig_n<64, MODE>(p, a, sign, s);
        case 128: return launch_contig_n<128, MODE>(p, a, sign, s);
        case 256: return launch_contig_n<256, MODE>(p, a, sign, s);
        case 512: return launch_contig_n<512, MODE>(p, a, sign, s);
        case 1024: return launch_contig_n<1024, MODE>(p, a, sign, s);
        case 2048: if constexpr (MODE == ZMODE_C2C) return launch_contig_n<2048, MODE>(p, a, sign, s); break;
    }
    fb_set_error("unsupported grid size (need a power of two, 16..2048)");
    return FB_ERR_UNSUPPORTED;
}

// ---- grids that are not powers of two: the plain generic passes of fb_fft_generic.h ------------------------------------
template <int MODE>
int launch_generic(fb_plan* p, GenericArgs<real_t>& a, int nouter, hipStream_t s) {
    if (!factor_smooth(a.n, a.rp)) { fb_set_error("unsupported grid size: nsamp must be even with prime factors 2, 3, 5 only"); return FB_ERR_UNSUPPORTED; }
    a.tw = p->tw.as<const cplx_t>();
    a.N = p->N;
    int TZ = (int)(65536 / ((size_t)2 * a.n * sizeof(cplx_t)));
    TZ = TZ < 1 ? 1 : (TZ > 8 ? 8 : TZ);
    const size_t lds = (size_t)2 * a.n * TZ * sizeof(cplx_t);
    int r = set_lds(k_fft_generic<real_t, MODE>, lds);
    if (r) return r;
    const unsigned tiles = (unsigned)((a.nlines + TZ - 1) / TZ);
    { FbProfScope _ps(p, a.pstride_in == 1 ? FBK_FFT_CONTIG : FBK_FFT_STRIDED, s);
    hipLaunchKernelGGL((k_fft_generic<real_t, MODE>), dim3(tiles, (unsigned)nouter), dim3(256), lds, s, a, TZ); }
    FB_LAUNCH_CHECK("k_fft_generic");
    return FB_OK;
}
// strided c2c pass in place over data with `ncols` contiguous columns: lines `stride` apart, tiles along `outer`
int generic_strided(fb_plan* p, cplx_t* d, long long stride, long long outer_stride, int ncols, int nouter, int sign, double scale,
                    hipStream_t s) {
    GenericArgs<real_t> a = {};
    a.in = d; a.out = d; a.n = p->N;
    a.pstride_in = a.pstride_out = stride; a.cstride_in = a.cstride_out = 1; a.ostride_in = a.ostride_out = outer_stride;
    a.nlines = ncols; a.sign = sign; a.scale = (real_t)scale;
    return launch_generic<GMODE_C2C>(p, a, nouter, s);
}
int generic_c2c(fb_plan* p, cplx_t* d, int sign, double scale, hipStream_t s) {
    const int N = p->N;
    const long long NN = (long long)N * N;
    int r = generic_strided(p, d, NN, N, N, N, sign, 1.0, s);                 // x lines, tiles over (y, z)
    if (!r) r = generic_strided(p, d, N, NN, N, N, sign, 1.0, s);             // y lines, tiles over (x, z)
    if (r) return r;
    GenericArgs<real_t> a = {};
    a.in = d; a.out = d; a.n = N; a.pstride_in = a.pstride_out = 1; a.cstride_in = a.cstride_out = N;
    a.nlines = (int)NN; a.sign = sign; a.scale = (real_t)scale;
    return launch_generic<GMODE_C2C>(p, a, 1, s);
}
int generic_r2c(fb_plan* p, const void* real_in, cplx_t* h, hipStream_t s) {
    const int N = p->N;
    const long long hplane = (long long)p->NR * p->NZP;
    GenericArgs<real_t> a = {};
    a.in = real_in; a.out = h; a.n = N / 2;
    a.pstride_in = 1; a.cstride_in = N; a.pstride_out = 1; a.cstride_out = p->NZP; a.skip_out = N;
    a.nlines = N * N; a.sign = -1; a.scale = (real_t)1;
    int r = launch_generic<GMODE_R2C>(p, a, 1, s);
    if (!r) r = generic_strided(p, h, p->NZP, hplane, p->NZV, N, -1, 1.0, s);       // y lines inside every x-plane
    if (!r) r = generic_strided(p, h, hplane, p->NZP, p->NZV, N, -1, 1.0, s);       // x lines
    return r;
}
int generic_c2r(fb_plan* p, cplx_t* h, void* real_out, double scale, hipStream_t s) {
    const int N = p->N;
    const long long hplane = (long long)p->NR * p->NZP;
    int r = generic_strided(p, h, hplane, p->NZP, p->NZV, N, +1, 1.0, s);
    if (!r) r = generic_strided(p, h, p->NZP, hplane, p->NZV, N, +1, 1.0, s);
    if (r) return r;
    GenericArgs<real_t> a = {};
    a.in = h; a.out = real_out; a.n = N / 2;
    a.pstride_in = 1; a.cstride_in = p->NZP; a.skip_in = N; a.pstride_out = 1; a.cstride_out = N;
    a.nlines = N * N; a.sign = +1; a.scale = (real_t)scale;
    return launch_generic<GMODE_C2R>(p, a, 1, s);
}

// the two strided views of a half spectrum [N][NR][NZP]
// packed: the work spectrum of a fused chain keeps the k_z = N/2 plane in the imaginary direction of the k_z = 0 plane
// (both are transforms of real 2-D fields, so X(k_z=0) + i X(k_z=N/2) loses nothing): N/2 columns instead of N/2 + 1,
// i.e. exactly N/32 full 16-column tiles per row instead of one more that is 15/16 padding (5.9 % of every strided
// pass at 512^3).  The layout never leaves the library: the generator writes it, the z passes read / write it, the
// binning pass untangles it (k_bin_packed_plane).  FB_PACKED=0 switches it off (tuning aid).
bool use_packed(const fb_plan* p) {
    static const int env = getenv("FB_PACKED") ? atoi(getenv("FB_PACKED")) : 1;
    return env != 0 && p->N >= 16;
}
StridedArgs<real_t> half_x(const fb_plan* p, cplx_t* h, bool packed = false) {
    StridedArgs<real_t> a{h, h, p->tw.as<const cplx_t>(), (long long)p->NR * p->NZP, (long long)p->NZP, packed ? p->N / 2 : p->NZV, (real_t)1};
    a.packed = packed;
    return a;
}
StridedArgs<real_t> half_y(const fb_plan* p, cplx_t* h, bool packed = false) {
    StridedArgs<real_t> a{h, h, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)p->NR * p->NZP, packed ? p->N / 2 : p->NZV, (real_t)1};
    a.packed = packed;
    return a;
}

// ---- the y and z passes of a half-spectrum transform, batch by batch over x-planes ------------------------------
// Both passes work inside one x-plane, so they can run plane batch by plane batch: a batch that stays in the 256 MiB
// Infinity Cache is read from HBM once and written once however many passes touch it, and the tile pattern of the
// strided pass itself copies ~25 % faster from there (tools/mall_copy.hip, profiles/r01g_mall_copy.txt).
// Measured at 512^3 (fp32), headline step: 757 -> 864 boxes/s with batches of 128 planes on the caller's stream.
// With FB_PLANE_STREAMS=2 alternate (smaller) batches go to an auxiliary stream of the plan, so that one batch's
// kernel boundaries overlap the other's kernels: +3 % while every launch carried a profiling event pair, nothing once
// those were thinned out, and per-kernel durations that no longer mean anything on their own; off by default.
//   FB_PLANE_BATCH   = planes per batch (0: whole box in one go; unset: sized to the cache)
//   FB_PLANE_STREAMS = 1 | 2 (unset: 2 from 1024^3 up)
struct PlaneBatches { int per, count, streams; };
PlaneBatches plane_batches(const fb_plan* p, size_t bytes_per_plane, bool whole_when_unset = false) {
    static const int env_b = getenv("FB_PLANE_BATCH") ? atoi(getenv("FB_PLANE_BATCH")) : -1;
    static const int env_s = getenv("FB_PLANE_STREAMS") ? atoi(getenv("FB_PLANE_STREAMS")) : 0;   // 0: by size
    const int N = p->N;
    // two streams pay from 1024^3 up (+5 %: 93.4 against 88.9 boxes/s at 1024^3, 9.45 against 8.95 at 2048^3), where
    // a batch is only a few planes and its launches are short; at 512^3 one stream does as well and keeps every
    // kernel's duration its own
    const int sel_s = p->plane_streams ? p->plane_streams : env_s;       // the plan's setting, else the environment's
    const int ns = sel_s ? (sel_s >= 2 ? 2 : 1) : (N >= 1024 ? 2 : 1);
    // working set of the batches in flight: measured optimum 288 MB for one stream (the boundaries between the
    // kernels of a batch cost as much as the cache misses of a slightly oversized batch), 2 x 112 MB for two
    const size_t budget = (size_t)(ns == 1 ? 288 : 112) << 20;
    int B = p->plane_batch >= 0 ? p->plane_batch : env_b;
    if (B < 0 && whole_when_unset) return PlaneBatches{N, 1, 1};
    if (B < 0) {
        B = ((size_t)N * bytes_per_plane <= ((size_t)320 << 20)) ? N : (int)(budget / bytes_per_plane);
        // 2048^3: three planes are 1.5 rounds of y-pass workgroups (9.26 /s); 4-16 planes: 9.45-9.52.  With the y passes in
        // 128-byte rows (round 4: 64 tiles per plane, resident workgroups) a launch wants several tiles per CU: 16-32 planes
        // 12.06-12.13 boxes/s against 11.78 with 4 (and 11.95 for the 64-byte-row form at its best, 4): profiles/r04_pass_bench_2048.txt
        const int min_planes = (N >= 2048 && sizeof(real_t) == 4) ? 16 : 4;
        if (B < min_planes) B = min_planes;
    }
    if (B <= 0 || B >= N) return PlaneBatches{N, 1, 1};
    int nb = (N + B - 1) / B;
    nb = (nb + ns - 1) / ns * ns;
    B = (N + nb - 1) / nb;
    return PlaneBatches{B, (N + B - 1) / B, ns};
}
int fork_streams(fb_plan* p, const PlaneBatches& pb, hipStream_t s) {
    if (pb.streams < 2) return FB_OK;
    if (!p->aux_stream) {
        FB_HIP(hipStreamCreateWithFlags(&p->aux_stream, hipStreamNonBlocking));
        FB_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
        FB_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    }
    FB_HIP(hipEventRecord(p->ev_fork, s));
    FB_HIP(hipStreamWaitEvent(p->aux_stream, p->ev_fork, 0));
    return FB_OK;
}
int join_streams(fb_plan* p, const PlaneBatches& pb, hipStream_t s) {
    if (pb.streams < 2) return FB_OK;
    FB_HIP(hipEventRecord(p->ev_join, p->aux_stream));
    FB_HIP(hipStreamWaitEvent(s, p->ev_join, 0));
    return FB_OK;
}

// ZM = ZMODE_C2R   : [inverse y pass,] half -> real
//      ZMODE_C2R2C : [inverse y pass,] half -> real (stored) -> half of (exp of) it [, forward y pass]
//      ZMODE_R2C   : real -> half [, forward y pass]
template <int ZM>
int yz_passes(fb_plan* p, cplx_t* h, const void* real_in, void* real_out, bool y_before, bool y_after, double scale,
              int pre_exp, hipStream_t s, bool packed = false) {
    const int N = p->N;
    const long long hplane = (long long)p->NR * p->NZP, rplane = (long long)N * N;
    const PlaneBatches pb = plane_batches(p, (size_t)hplane * sizeof(cplx_t) + (size_t)rplane * sizeof(real_t));
    int r = FB_OK;
    if (pre_exp && pb.count > 1) {       // one allocation for every batch's block sums (no reallocation mid-way)
        r = p->exp_partials.ensure(((size_t)rplane + (size_t)pb.count) * sizeof(double));
        if (r) return r;
    }
    r = fork_streams(p, pb, s);
    if (r) return r;
    p->exp_base = 0;
    for (int b = 0; b < pb.count && !r; ++b) {
        const int p0 = b * pb.per, cnt = (p0 + pb.per <= N) ? pb.per : N - p0;
        hipStream_t st = (pb.streams > 1 && (b & 1)) ? p->aux_stream : s;
        cplx_t* hb = h + p0 * hplane;
        if (y_before) r = launch_plain(p, N, half_y(p, hb, packed), cnt, +1, st);
        if (r) break;
        if (ZM == ZMODE_R2C) {
            ContigArgs<real_t> az{reinterpret_cast<const real_t*>(real_in) + p0 * rplane, hb, p->tw.as<const cplx_t>(), (long long)N,
                                  (long long)p->NZP, 0, N, cnt * (long long)N, (real_t)1, pre_exp, nullptr, nullptr, packed};
            r = launch_contig<ZM>(p, N / 2, az, -1, st);
        } else {
            ContigArgs<real_t> az{hb, real_out ? reinterpret_cast<real_t*>(real_out) + p0 * rplane : nullptr, p->tw.as<const cplx_t>(), (long long)p->NZP,
                                  (long long)N, N, 0, cnt * (long long)N, (real_t)scale, pre_exp, nullptr,
                                  ZM == ZMODE_C2R2C ? hb : nullptr, packed};
            r = launch_contig<ZM>(p, N / 2, az, +1, st);
        }
        if (r) break;
        p->exp_base = p->exp_rows;
        if (y_after) r = launch_plain(p, N, half_y(p, hb, packed), cnt, -1, st);
    }
    p->exp_base = 0;
    const int rj = join_streams(p, pb, s);
    return r ? r : rj;
}

// last forward pass of a P(k) estimate: x pass with the shell binning fused (nothing written) and the column sums
// -> results[2 nbins + 1] = (sum |dk|^2, sum |dk|^4) per bin, then sum(exp(x)) of the log-normal mean (or 0)
int bin_x_pass(fb_plan* p, cplx_t* h, bool packed, int pre_exp, double* results, hipStream_t s) {
    const int N = p->N, nb = p->nbins;
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.thr = p->thr; op.bins = p->bins; op.nbins = nb; op.namb = p->namb; op.store = 0;
    for (int q = 0; q < 8; ++q) op.amb[q] = p->amb[q];
    op.plane_out = packed ? p->plane_buf.as<cplx_t>() : nullptr;
    int r = launch_strided<SMODE_BIN>(p, N, half_x(p, h, packed), N, -1, op, s);
    if (r) return r;
    if (packed) {
        BinGeom bg;
        bg.bins = p->bins; bg.thr = p->use_thr ? p->thr : nullptr; bg.nbins = nb; bg.namb = p->namb;
        for (int q = 0; q < 8; ++q) bg.amb[q] = p->amb[q];
        const size_t lds = (size_t)nb * sizeof(double) + (size_t)8 * nb * sizeof(double) + (size_t)nb * sizeof(int);
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_bin_packed_plane<real_t>, dim3(N), dim3(256), lds, s, p->plane_buf.as<const cplx_t>(),
                           op.g, bg, p->bin_partials, p->bin_rows, p->bin_rows_main); }
        FB_LAUNCH_CHECK("k_bin_packed_plane");
    }
    { FbProfScope _ps(p, FBK_BIN, s);       // bin sums and (workgroup 2 nb) the sum of exp(), or 0, in one launch
    hipLaunchKernelGGL(k_sum_columns, dim3(2 * nb + 1), dim3(1024), 0, s, p->bin_partials, p->bin_rows, 2 * nb, results,
                       pre_exp ? p->exp_partials : nullptr, (long long)p->exp_rows, 0LL); }
    FB_LAUNCH_CHECK("k_sum_columns");
    return FB_OK;
}

// last forward pass of "P(k) of the filtered field": the x pass multiplies by T, keeps the filtered spectrum (inverse_x:
// already transformed back along x) and bins it
int filtered_x_pass(fb_plan* p, cplx_t* h, int kind, const double* prm, const void* table, double* results, int inverse_x,
                    hipStream_t s) {
    const int N = p->N, nb = p->nbins;
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.thr = p->thr; op.bins = p->bins; op.nbins = nb; op.namb = p->namb; op.store = inverse_x ? 2 : 1;
    for (int q = 0; q < 8; ++q) op.amb[q] = p->amb[q];
    op.filt.kind = kind; op.filt.table = table;
    for (int q = 0; q < 4; ++q) op.filt.p[q] = prm ? prm[q] : 0.0;
    op.kperp_tab = p->kperp_tab;
    int r = launch_strided<SMODE_BINF>(p, N, half_x(p, h), N, -1, op, s);
    if (r) return r;
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_sum_columns, dim3(2 * nb + 1), dim3(1024), 0, s, p->bin_partials, p->bin_rows, 2 * nb, results,
                       (const double*)nullptr, 0LL, 0LL); }
    FB_LAUNCH_CHECK("k_sum_columns");
    return FB_OK;
}
int filter_args_ok(const fb_plan* p, int kind, const void* table) {
    if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    if (kind < 0 || kind > FILT_TOPHAT) { fb_set_error("unknown filter kind"); return FB_ERR_INVALID; }
    if (kind == FILT_TOPHAT) {      // (k_apply_filter / k_bin_rows evaluate it; the fused pass is compiled without it)
        fb_set_error("the fused filtering pass takes FB_FILT_TABLE, _BEAM_HIGHPASS and _WEDGE; apply FB_FILT_TOPHAT with fb_apply_filter");
        return FB_ERR_UNSUPPORTED;
    }
    if (kind == FILT_TABLE && !table) { fb_set_error("FB_FILT_TABLE needs a device table"); return FB_ERR_INVALID; }
    return FB_OK;
}

template <int E_>
int launch_rsd_turn(fb_plan* p, const RsdTurnArgs<real_t>& a, hipStream_t s) {
    if constexpr (sizeof(real_t) == 4) {
        constexpr size_t lds = rsd_turn_lds<E_>();
        int r = set_lds(k_rsd_turn<real_t, E_>, lds);
        if (r) return r;
        const unsigned nb = (unsigned)((a.nlines + FB_RSDT_WAVES - 1) / FB_RSDT_WAVES);
        { FbProfScope _ps(p, FBK_RSD, s);
        hipLaunchKernelGGL((k_rsd_turn<real_t, E_>), dim3(nb), dim3(64 * FB_RSDT_WAVES), lds, s, a); }
        FB_LAUNCH_CHECK("k_rsd_turn");
        return FB_OK;
    } else {
        fb_set_error("the fused redshift-space z pass is built for single-precision plans");
        return FB_ERR_UNSUPPORTED;
    }
}

}  // namespace

#define FB_CAT2(a, b) a##b
#define FB_CAT(a, b) FB_CAT2(a, b)

// full complex [N][N][N], in place
int FB_CAT(fbi_fft_c2c_, FB_SUFFIX)(fb_plan* p, void* data, int sign, double scale, hipStream_t s) {
    if (p->generic) return generic_c2c(p, reinterpret_cast<cplx_t*>(data), sign, scale, s);
    const int N = p->N;
    const long long NN = (long long)N * N;
    cplx_t* d = reinterpret_cast<cplx_t*>(data);
    const cplx_t* tw = p->tw.as<const cplx_t>();
    StridedArgs<real_t> ax{d, d, tw, NN, (long long)N, N, (real_t)1};
    int r = launch_plain(p, N, ax, N, sign, s);          // x lines, tiles over (y, z)
    if (r) return r;
    // y lines (tiles over (x, z)) and z lines, plane batch by plane batch (see yz_passes)
    const PlaneBatches pb = plane_batches(p, (size_t)NN * sizeof(cplx_t));
    r = fork_streams(p, pb, s);
    if (r) return r;
    for (int b = 0; b < pb.count && !r; ++b) {
        const int p0 = b * pb.per, cnt = (p0 + pb.per <= N) ? pb.per : N - p0;
        hipStream_t st = (pb.streams > 1 && (b & 1)) ? p->aux_stream : s;
        cplx_t* db = d + p0 * NN;
        StridedArgs<real_t> ay{db, db, tw, (long long)N, NN, N, (real_t)1};
        r = launch_plain(p, N, ay, cnt, sign, st);
        if (r) break;
        ContigArgs<real_t> az{db, db, tw, (long long)N, (long long)N, 0, 0, cnt * (long long)N, (real_t)scale, 0, nullptr, nullptr};
        r = launch_contig<ZMODE_C2C>(p, N, az, sign, st);
    }
    const int rj = join_streams(p, pb, s);
    return r ? r : rj;
}

// complex [N][N][N] cube, transforms over axes 0 and 1 only (every z / frequency channel its own 2-D transform):
// np.fft.fftn(cube, axes=[0, 1]) (sign -1, scale 1) or ifftn (sign +1, scale 1/N^2).  Two strided passes.
namespace {
// the same for a cube [N][N][nz] with any number of channels nz
// y_planes = (first, count): the y pass only touches those x-planes -- run first when the others are known to be zero
// (forward transform of a zero-padded cube), last when the others are not wanted (inverse, cropped afterwards)
int fft_axes01_nz(fb_plan* p, cplx_t* d, int nz, int sign, double scale, hipStream_t s, bool y_first = false,
                  int y_plane0 = 0, int y_planes = -1) {
    const int N = p->N;
    const long long plane = (long long)N * nz;
    const cplx_t* tw = p->tw.as<const cplx_t>();
    if (y_planes < 0) y_planes = N;
    StridedArgs<real_t> ax{d, d, tw, plane, (long long)nz, nz, (real_t)1};
    cplx_t* dy = d + y_plane0 * plane;
    StridedArgs<real_t> ay{dy, dy, tw, (long long)nz, plane, nz, (real_t)scale};
    // (a grid that is not a power of two: the same two passes through the plain generic kernel)
    auto pass = [&](const StridedArgs<real_t>& a, int nouter) {
        if (p->generic) return generic_strided(p, a.out, a.stride, a.outer_stride, a.ncols, nouter, sign, (double)a.scale, s);
        return launch_plain(p, N, a, nouter, sign, s);
    };
    int r = y_first ? pass(ay, y_planes)      // y lines, tiles over (x, z)
                    : pass(ax, N);            // x lines, tiles over (y, z)
    if (r) return r;
    return y_first ? pass(ax, N) : pass(ay, y_planes);
}
}  // namespace
int FB_CAT(fbi_fft_axes01_, FB_SUFFIX)(fb_plan* p, void* data, int sign, double scale, hipStream_t s) {
    return fft_axes01_nz(p, reinterpret_cast<cplx_t*>(data), p->N, sign, scale, s);
}

// BeamModel.convolve_fft / convolve_real (fastbox/beams.py:63-137) of an n^3 field with an n^3 beam cube, channel by
// channel, on the plan of the TRANSFORM size M = p->N: M = 2n (zero-padded, linear convolution as
// scipy.signal.fftconvolve(beam, field, mode='same', axes=[0, 1])) or M = n (periodic, as convolve2d(...,
// boundary='wrap')).  work_a, work_b: complex [M][M][n].  out = conv / sum_xy(beam) per channel.
int FB_CAT(fbi_beam_convolve_, FB_SUFFIX)(fb_plan* p, const void* field, const void* beam, void* work_a, void* work_b,
                                          void* out, int flags, hipStream_t s) {
    const bool periodic = flags & 1, beam_ready = flags & 2;
    const int M = p->N, n = periodic ? M : M / 2;
    const int off = (n - 1) / 2;
    cplx_t* a = reinterpret_cast<cplx_t*>(work_a);
    cplx_t* b = reinterpret_cast<cplx_t*>(work_b);
    const long long count = (long long)M * M * n;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_beam_embed<real_t>, dim3((unsigned)(M * M)), dim3(256), 0, s, reinterpret_cast<const real_t*>(field), a, n, M);
    if (!beam_ready)
        hipLaunchKernelGGL(k_beam_embed<real_t>, dim3((unsigned)(M * M)), dim3(256), 0, s, reinterpret_cast<const real_t*>(beam), b, n, M); }
    FB_LAUNCH_CHECK("k_beam_embed");
    // zero-padded: the y lines of the planes x >= n are all zero, so the y pass runs first and only over x < n
    int r = fft_axes01_nz(p, a, n, -1, 1.0, s, true, 0, n);
    if (r) return r;
    if (!beam_ready) r = fft_axes01_nz(p, b, n, -1, 1.0, s, true, 0, n);
    if (r) return r;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_beam_multiply<real_t>, dim3(4096), dim3(256), 0, s, a, b, count); }
    FB_LAUNCH_CHECK("k_beam_multiply");
    // only the planes x in [off, off + n) survive the crop: x pass first, then the y pass over those planes alone
    // (all of them when the transform is periodic: the crop wraps)
    r = fft_axes01_nz(p, a, n, +1, 1.0 / ((double)M * M), s, false, periodic ? 0 : off, periodic ? M : n);
    if (r) return r;
    { FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL(k_beam_crop<real_t>, dim3((unsigned)(n * n)), dim3(256), 0, s, a, b, reinterpret_cast<real_t*>(out), n, M,
                       off); }
    FB_LAUNCH_CHECK("k_beam_crop");
    return FB_OK;
}

// complex [N][N] map, in place: lines along y (contiguous) then along x (stride N)
int FB_CAT(fbi_fft2d_c2c_, FB_SUFFIX)(fb_plan* p, void* data, int sign, double scale, hipStream_t s) {
    const int N = p->N;
    cplx_t* d = reinterpret_cast<cplx_t*>(data);
    if (p->generic) {        // lines along y: the N rows are the "columns" of a pass whose points are 1 apart; then lines along x
        GenericArgs<real_t> a = {};
        a.in = d; a.out = d; a.n = N; a.pstride_in = a.pstride_out = 1; a.cstride_in = a.cstride_out = N;
        a.nlines = N; a.sign = sign; a.scale = (real_t)scale;
        int r = launch_generic<GMODE_C2C>(p, a, 1, s);
        if (r) return r;
        return generic_strided(p, d, N, 0LL, N, 1, sign, 1.0, s);
    }
    const cplx_t* tw = p->tw.as<const cplx_t>();
    ContigArgs<real_t> ay{d, d, tw, (long long)N, (long long)N, 0, 0, (long long)N, (real_t)scale, 0, nullptr, nullptr};
    int r = launch_contig<ZMODE_C2C>(p, N, ay, sign, s);
    if (r) return r;
    StridedArgs<real_t> ax{d, d, tw, (long long)N, 0LL, N, (real_t)1};
    return launch_plain(p, N, ax, 1, sign, s);
}

// real [N][N][N] -> half spectrum [N][N][NZP], forward, unnormalised (numpy fftn)
int FB_CAT(fbi_fft_r2c_, FB_SUFFIX)(fb_plan* p, const void* real_in, void* half_out, int pre_exp, hipStream_t s) {
    if (p->generic) {
        if (pre_exp) { fb_set_error("the fused log-normal transform needs a power-of-two grid (use fb_lognormal, then fb_fft_r2c)"); return FB_ERR_UNSUPPORTED; }
        return generic_r2c(p, real_in, reinterpret_cast<cplx_t*>(half_out), s);
    }
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_out);
    int r = yz_passes<ZMODE_R2C>(p, h, real_in, nullptr, false, true, 1.0, pre_exp, s);
    if (r) return r;
    return launch_plain(p, N, half_x(p, h), N, -1, s);
}

// half spectrum (destroyed) -> real, inverse; scale = 1/N^3 reproduces numpy ifftn(...).real
int FB_CAT(fbi_fft_c2r_, FB_SUFFIX)(fb_plan* p, void* half_inout, void* real_out, double scale, hipStream_t s) {
    if (p->generic) return generic_c2r(p, reinterpret_cast<cplx_t*>(half_inout), real_out, scale, s);
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_inout);
    int r = launch_plain(p, N, half_x(p, h), N, +1, s);
    if (r) return r;
    return yz_passes<ZMODE_C2R>(p, h, nullptr, real_out, true, false, scale, 0, s);
}

// the y and z passes of fbi_fft_c2r_: for a half spectrum whose x lines have been transformed already
// (fbi_power_filtered_ with inverse_x)
int FB_CAT(fbi_fft_c2r_yz_, FB_SUFFIX)(fb_plan* p, void* half_inout, void* real_out, double scale, hipStream_t s) {
    cplx_t* h = reinterpret_cast<cplx_t*>(half_inout);
    return yz_passes<ZMODE_C2R>(p, h, nullptr, real_out, true, false, scale, 0, s);
}

// realise_density, throughput mode (box.py:161-187): the generator is fused into the x pass,
// so the coloured half spectrum is written once and never read back by a separate kernel.
int FB_CAT(fbi_realise_fused_, FB_SUFFIX)(fb_plan* p, uint64_t seed, uint64_t real, void* work_half, void* real_out,
                                          double scale, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    if (int ra = gen_amplitude(p, op)) return ra;
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    const bool packed = use_packed(p);
    int r = launch_strided<SMODE_GEN>(p, N, half_x(p, h, packed), N, +1, op, s);
    if (r) return r;
    return yz_passes<ZMODE_C2R>(p, h, nullptr, real_out, true, false, scale, 0, s, packed);
}

// Velocity component comp of the same realisation, in real space: Re ifftn(i fac delta_k k_c / k^2)
// (box.py:251-284 followed by the caller's ifftn(...).real).  The counter-based generator reproduces
// delta_k inside the first pass, so neither delta_k nor v(k) is ever stored.  Multiplying by the odd,
// imaginary factor commutes with the Hermitian projection the c2r pass applies to the k_z = 0, N/2 planes.
int FB_CAT(fbi_realise_velocity_fused_, FB_SUFFIX)(fb_plan* p, uint64_t seed, uint64_t real, int comp, double fac,
                                                   void* work_half, void* real_out, double scale, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    if (int ra = gen_amplitude(p, op)) return ra;
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    op.vel_on = 1; op.vel_comp = comp; op.vel_fac = fac;
    const bool packed = use_packed(p);
    int r = launch_strided<SMODE_GEN>(p, N, half_x(p, h, packed), N, +1, op, s);
    if (r) return r;
    return yz_passes<ZMODE_C2R>(p, h, nullptr, real_out, true, false, scale, 0, s, packed);
}

// Deferred realisation: generator + x pass now, the y and z passes later (plane batch by plane batch, see
// yz_passes), either alone (fbi_realise_finish) or together with the first passes of the power spectrum
// (fbi_power_from_pending).
int FB_CAT(fbi_realise_begin_, FB_SUFFIX)(fb_plan* p, uint64_t seed, uint64_t real, void* work_half, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    if (int ra = gen_amplitude(p, op)) return ra;
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    return launch_strided<SMODE_GEN>(p, N, half_x(p, h, use_packed(p)), N, +1, op, s);     // work_half: packed (see half_x)
}
int FB_CAT(fbi_realise_finish_, FB_SUFFIX)(fb_plan* p, void* work_half, void* real_out, double scale, hipStream_t s) {
    return yz_passes<ZMODE_C2R>(p, reinterpret_cast<cplx_t*>(work_half), nullptr, real_out, true, false, scale, 0, s,
                                use_packed(p));
}
// work_half holds the spectrum after the inverse x pass: per plane batch the inverse y pass, one fused z pass that
// writes the real field and turns work_half into the forward z spectrum of (exp of) it, and the forward y pass;
// then x(BIN).
int FB_CAT(fbi_power_from_pending_, FB_SUFFIX)(fb_plan* p, void* work_half, void* real_out, double scale, int pre_exp,
                                               double* results, hipStream_t s) {
    if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    const bool packed = use_packed(p);
    int r = yz_passes<ZMODE_C2R2C>(p, h, nullptr, real_out, true, true, scale, pre_exp, s, packed);
    if (r) return r;
    return bin_x_pass(p, h, packed, pre_exp, results, s);
}

// binned_power_spectrum(delta_x=...) (box.py:736-764) for cubic boxes: r2c with the shell
// binning fused into the last pass.  results[2*nbins+1] = (sum |dk|^2, sum |dk|^4) per bin,
// then sum(exp(x)) when pre_exp (0 otherwise).  The spectrum is written only if `store`.
int FB_CAT(fbi_power_fused_, FB_SUFFIX)(fb_plan* p, const void* real_in, void* work_half, int pre_exp, int store,
                                        double* results, hipStream_t s) {
    if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    const int N = p->N, nb = p->nbins;
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    const bool packed = !store && use_packed(p);
    int r = yz_passes<ZMODE_R2C>(p, h, real_in, nullptr, false, true, 1.0, pre_exp, s, packed);
    if (r) return r;
    if (store) {          // keep fftn(real_in): plain last pass, then the stand-alone binning kernel
        r = launch_plain(p, N, half_x(p, h), N, -1, s);
        if (r) return r;
        r = FB_CAT(fbi_bin_power_, FB_SUFFIX)(p, h, 1, -1, nullptr, nullptr, results, s);
        if (r) return r;
        if (!pre_exp) { FB_HIP(hipMemsetAsync(results + 2 * nb, 0, sizeof(double), s)); return FB_OK; }
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(1), dim3(256), 0, s, p->exp_partials, p->exp_rows, 1, results + 2 * nb, (const double*)nullptr, 0LL, 0LL); }
        FB_LAUNCH_CHECK("k_sum_columns");
        return FB_OK;
    }
    return bin_x_pass(p, h, packed, pre_exp, results, s);
}

// P(k) of ifftn(fftn(real_in) * T(k_perp, k_par)) for a real, k_par-even filter (apply_transfer_fn then
// binned_power_spectrum, box.py:356-381, :696-768): r2c + y pass, then the x pass multiplies by T, writes
// the FILTERED spectrum to filtered_half (for the inverse transform that delivers the field) and bins it.
// inverse_x: filtered_half receives the filtered spectrum already transformed back along x (fbi_fft_c2r_yz_ finishes it)
int FB_CAT(fbi_power_filtered_, FB_SUFFIX)(fb_plan* p, const void* real_in, void* filtered_half, int kind,
                                           const double* prm, const void* table, double* results, int inverse_x,
                                           hipStream_t s) {
    if (int rc = filter_args_ok(p, kind, table)) return rc;
    cplx_t* h = reinterpret_cast<cplx_t*>(filtered_half);
    int r = yz_passes<ZMODE_R2C>(p, h, real_in, nullptr, false, true, 1.0, 0, s);
    if (r) return r;
    return filtered_x_pass(p, h, kind, prm, table, results, inverse_x, s);
}

// Velocity component of a device-generator realisation, deferred like fbi_realise_begin_: generator + x pass now
// (work_half: packed), the y and z passes by fbi_realise_finish_ -- or by fbi_power_redshift_space_ below.
int FB_CAT(fbi_realise_velocity_begin_, FB_SUFFIX)(fb_plan* p, uint64_t seed, uint64_t real, int comp, double fac,
                                                   void* work_half, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(work_half);
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    if (int ra = gen_amplitude(p, op)) return ra;
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    op.vel_on = 1; op.vel_comp = comp; op.vel_fac = fac;
    return launch_strided<SMODE_GEN>(p, N, half_x(p, h, use_packed(p)), N, +1, op, s);
}

// redshift_space_density of two pending realisations (delta, v_z: generator + x pass done) followed by the forward
// transform of the result and its P(k) -- with a k_perp / k_par filter in between when kind >= 0 (box.py:384-438, then
// :356-381 and :696-768; BASELINE configs[2]).  Per plane batch: the inverse y passes of both work spectra, ONE z pass
// (k_rsd_turn: both inverse z transforms, the remap, the forward z transform; delta_x written to real_d_out unless
// null), the forward y pass; then the x pass that (filters, stores to out_half and) bins.  Both work spectra are
// destroyed.  kind < 0: no filter, nothing stored (out_half is work space).
int FB_CAT(fbi_power_redshift_space_, FB_SUFFIX)(fb_plan* p, void* work_d, void* work_v, void* real_d_out, void* out_half,
                                                 double scale, double Hz, double sigma_nl, uint64_t seed, int nearest,
                                                 int kind, const double* prm, const void* table, double* results,
                                                 int inverse_x, hipStream_t s) {
    if (kind >= 0) { if (int rc = filter_args_ok(p, kind, table)) return rc; }
    else if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    const int N = p->N;
    if (sizeof(real_t) != 4 || N < 64 || N > 512) {
        fb_set_error("the fused redshift-space pass needs a single-precision plan with 64 <= N <= 512");
        return FB_ERR_UNSUPPORTED;
    }
    cplx_t* hd = reinterpret_cast<cplx_t*>(work_d);
    cplx_t* hv = reinterpret_cast<cplx_t*>(work_v);
    cplx_t* ho = reinterpret_cast<cplx_t*>(out_half);
    const bool packed = use_packed(p);
    const long long hplane = (long long)p->NR * p->NZP, rplane = (long long)N * N;
    // Plane batches: the fused z pass is bound by LDS and issue slots, not by memory, so a batch resident in the Infinity
    // Cache buys it nothing and every batch costs four kernel boundaries: one box on the GPU runs the whole box per pass
    // (512^3: 2.79 against 2.99 ms per chain).  Several boxes on their own streams are told their share
    // (fb_set_plane_batching) and then do better with it -- the boundaries of one hide behind the kernels of the other
    // (two boxes: 2.52 against 2.65 ms).
    const PlaneBatches pb = plane_batches(p, (size_t)3 * hplane * sizeof(cplx_t) + (size_t)rplane * sizeof(real_t), true);
    int r = fork_streams(p, pb, s);
    if (r) return r;
    for (int b = 0; b < pb.count && !r; ++b) {
        const int p0 = b * pb.per, cnt = (p0 + pb.per <= N) ? pb.per : N - p0;
        hipStream_t st = (pb.streams > 1 && (b & 1)) ? p->aux_stream : s;
        r = launch_plain(p, N, half_y(p, hd + p0 * hplane, packed), cnt, +1, st);
        if (r) break;
        r = launch_plain(p, N, half_y(p, hv + p0 * hplane, packed), cnt, +1, st);
        if (r) break;
        RsdTurnArgs<real_t> a = {};
        a.in_d = hd + p0 * hplane; a.in_v = hv + p0 * hplane;
        a.dx_out = real_d_out ? reinterpret_cast<real_t*>(real_d_out) + p0 * rplane : nullptr;
        a.out = ho + p0 * hplane;
        a.tw = p->tw.as<const cplx_t>(); a.zgrid = p->zgrid; a.pitch = p->NZP;
        a.nlines = cnt * (long long)N; a.line0 = p0 * (long long)N;
        a.scale_d = (real_t)scale; a.scale_v = (real_t)scale; a.packed_in = packed ? 1 : 0;
        a.Hz = Hz; a.sigma_nl = sigma_nl;
        a.rkey.k[0] = (uint32_t)seed; a.rkey.k[1] = (uint32_t)(seed >> 32); a.rkey.k[2] = 0; a.rkey.k[3] = 0;
        a.nearest = nearest;
        switch (N) {
            case 64: r = launch_rsd_turn<1>(p, a, st); break;
            case 128: r = launch_rsd_turn<2>(p, a, st); break;
            case 256: r = launch_rsd_turn<4>(p, a, st); break;
            default: r = launch_rsd_turn<8>(p, a, st); break;
        }
        if (r) break;
        r = launch_plain(p, N, half_y(p, ho + p0 * hplane), cnt, -1, st);
    }
    const int rj = join_streams(p, pb, s);
    if (r || rj) return r ? r : rj;
    if (kind < 0) return bin_x_pass(p, ho, false, 0, results, s);
    return filtered_x_pass(p, ho, kind, prm, table, results, inverse_x, s);
}

// tuning aid: one strided pass over a half spectrum. axis 0 = x, 1 = y; mode 0 plain (in place),
// 1 generator (x only), 2 binning without store (x only).
int FB_CAT(fbi_debug_pass_, FB_SUFFIX)(fb_plan* p, void* half, int axis, int mode, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half);
    const bool packed = use_packed(p) && mode % 10 != 2;   // the layout the production chains run (16 tiles per row at 512);
                                                            // the binning pass of a packed spectrum needs bin_x_pass's plane buffer
    StridedArgs<real_t> a = axis == 0 ? half_x(p, h, packed) : half_y(p, h, packed);
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    p->debug_no_mem = (mode >= 10);
    mode %= 10;
    struct Reset { fb_plan* q; ~Reset() { q->debug_no_mem = 0; } } reset{p};
    if (mode == 1) {
        op.amp.shell = p->amp_shell.as<const real_t>();
        op.amp.dense = nullptr;
        op.amp.sym = p->amp_sym.as<const real_t>();
        if (!op.amp.shell) { fb_set_error("amplitude shells not set"); return FB_ERR_STATE; }
#ifdef FB_STAMPS
        {
            int r = p->bin_partials.ensure(((size_t)N * 64 * 32 + 4096) * sizeof(double));
            if (r) return r;
            op.bins = p->bin_partials;          // time stamps (the generator does not read bins)
        }
#endif
        return launch_strided<SMODE_GEN>(p, N, a, N, +1, op, s);
    }
    if (mode == 2) {
        if (!p->nbins || !p->use_thr) { fb_set_error("bins not set"); return FB_ERR_STATE; }
        op.thr = p->thr; op.bins = p->bins; op.nbins = p->nbins; op.namb = p->namb; op.store = 0;
        for (int q = 0; q < 8; ++q) op.amb[q] = p->amb[q];
        return launch_strided<SMODE_BIN>(p, N, a, N, -1, op, s);
    }
#ifdef FB_STAMPS
    {   // diagnostic build: time stamps land in bin_partials (8 int64 per workgroup)
        int r = p->bin_partials.ensure(((size_t)N * 64 * 32 + 4096) * sizeof(double));
        if (r) return r;
        op.bins = p->bin_partials;
        return launch_strided<SMODE_PLAIN>(p, N, a, N, -1, op, s);
    }
#endif
    return launch_plain(p, N, a, N, -1, s);
}


// ---- slab-decomposed 3-D FFT (one x-slab / k_y-slab per rank; the exchange is done by the host) ------
namespace {
StridedArgs<real_t> slab_y(const fb_plan* p, cplx_t* h) {       // x-slab [nxl][NR][NZP]: y lines
    return StridedArgs<real_t>{h, h, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)p->NR * p->NZP, p->NZV, (real_t)1};
}
StridedArgs<real_t> slab_x(const fb_plan* p, cplx_t* k, int nyl) {  // k-space slab [N][nyl][NZP]: x lines
    return StridedArgs<real_t>{k, k, p->tw.as<const cplx_t>(), (long long)nyl * p->NZP, (long long)p->NZP, p->NZV, (real_t)1};
}
}  // namespace

int FB_CAT(fbi_slab_forward_local_, FB_SUFFIX)(fb_plan* p, const void* real_local, void* half_local, int nxl,
                                               int pre_exp, double* expsum, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    ContigArgs<real_t> az{real_local, h, p->tw.as<const cplx_t>(), (long long)N, (long long)p->NZP, 0, N,
                          (long long)nxl * N, (real_t)1, pre_exp, nullptr, nullptr};
    int r = launch_contig<ZMODE_R2C>(p, N / 2, az, -1, s);
    if (r) return r;
    if (pre_exp && expsum) {
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(1), dim3(256), 0, s, p->exp_partials, p->exp_rows, 1, expsum, (const double*)nullptr, 0LL, 0LL); }
        FB_LAUNCH_CHECK("k_sum_columns");
    }
    return launch_plain(p, N, slab_y(p, h), nxl, -1, s);
}

int FB_CAT(fbi_slab_inverse_local_, FB_SUFFIX)(fb_plan* p, void* half_local, void* real_local, int nxl, double scale,
                                               hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    int r = launch_plain(p, N, slab_y(p, h), nxl, +1, s);
    if (r) return r;
    ContigArgs<real_t> az{h, real_local, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)N, N, 0,
                          (long long)nxl * N, (real_t)scale, 0, nullptr, nullptr};
    return launch_contig<ZMODE_C2R>(p, N / 2, az, +1, s);
}

// The same two with the pack / unpack folded into the y pass: `xbuf` is the [rank][x][k_y in rank][k_z] buffer of the
// all-to-all.  Needs nparts | (points per thread of a y line), true for 1, 2, 4, 8 ranks (16 at N = 2048).
namespace {
int slab_blocking(StridedArgs<real_t>& a, const fb_plan* p, int nxl, int nparts, bool out_side) {
    const int N = p->N, E = strided_elems(N);
    int m = E / nparts, shift = 0;
    if (nparts < 1 || m * nparts != E) { fb_set_error("fused slab exchange needs the rank count to divide the points per thread"); return FB_ERR_UNSUPPORTED; }
    while ((1 << shift) < m) ++shift;
    const long long nyl = N / nparts;
    a.blk_shift = shift;
    a.blk_stride = (long long)nxl * nyl * p->NZP;                 // one rank's block
    if (out_side) { a.blk_out = 1; a.out_outer_stride = nyl * p->NZP; }
    else { a.blk_in = 1; a.out_outer_stride = a.outer_stride; a.outer_stride = nyl * p->NZP; }
    return FB_OK;
}
}  // namespace

int FB_CAT(fbi_slab_forward_packed_, FB_SUFFIX)(fb_plan* p, const void* real_local, void* half_local, void* xbuf,
                                                int nxl, int nparts, int pre_exp, double* expsum, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    ContigArgs<real_t> az{real_local, h, p->tw.as<const cplx_t>(), (long long)N, (long long)p->NZP, 0, N,
                          (long long)nxl * N, (real_t)1, pre_exp, nullptr, nullptr};
    int r = launch_contig<ZMODE_R2C>(p, N / 2, az, -1, s);
    if (r) return r;
    if (pre_exp && expsum) {
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(1), dim3(256), 0, s, p->exp_partials, p->exp_rows, 1, expsum, (const double*)nullptr, 0LL, 0LL); }
        FB_LAUNCH_CHECK("k_sum_columns");
    }
    StridedArgs<real_t> ay = slab_y(p, h);
    ay.out = reinterpret_cast<cplx_t*>(xbuf);
    r = slab_blocking(ay, p, nxl, nparts, true);
    if (r) return r;
    return launch_plain(p, N, ay, nxl, -1, s);
}

int FB_CAT(fbi_slab_inverse_packed_, FB_SUFFIX)(fb_plan* p, const void* xbuf, void* half_local, void* real_local, int nxl,
                                                int nparts, double scale, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    StridedArgs<real_t> ay = slab_y(p, h);
    ay.in = reinterpret_cast<const cplx_t*>(xbuf);
    int r = slab_blocking(ay, p, nxl, nparts, false);
    if (r) return r;
    r = launch_plain(p, N, ay, nxl, +1, s);
    if (r) return r;
    ContigArgs<real_t> az{h, real_local, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)N, N, 0,
                          (long long)nxl * N, (real_t)scale, 0, nullptr, nullptr};
    return launch_contig<ZMODE_C2R>(p, N / 2, az, +1, s);
}

// realise_density's local half and binned_power_spectrum's local half in one go: y pass out of the receive
// buffer, ONE z pass that writes the real slab and the forward z spectrum of (exp of) it, y pass into the send
// buffer.  The real slab is written once and never read back (as fbi_power_from_pending on a single GPU).
int FB_CAT(fbi_slab_turnaround_, FB_SUFFIX)(fb_plan* p, const void* recvbuf, void* half_local, void* real_local,
                                            void* sendbuf, int nxl, int nparts, double scale, int pre_exp,
                                            double* expsum, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    StridedArgs<real_t> ai = slab_y(p, h);
    ai.in = reinterpret_cast<const cplx_t*>(recvbuf);
    int r = slab_blocking(ai, p, nxl, nparts, false);
    if (r) return r;
    r = launch_plain(p, N, ai, nxl, +1, s);
    if (r) return r;
    ContigArgs<real_t> az{h, real_local, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)N, N, 0,
                          (long long)nxl * N, (real_t)scale, pre_exp, nullptr, h};
    r = launch_contig<ZMODE_C2R2C>(p, N / 2, az, +1, s);
    if (r) return r;
    if (pre_exp && expsum) {
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(1), dim3(256), 0, s, p->exp_partials, p->exp_rows, 1, expsum, (const double*)nullptr, 0LL, 0LL); }
        FB_LAUNCH_CHECK("k_sum_columns");
    }
    StridedArgs<real_t> ao = slab_y(p, h);
    ao.out = reinterpret_cast<cplx_t*>(sendbuf);
    r = slab_blocking(ao, p, nxl, nparts, true);
    if (r) return r;
    return launch_plain(p, N, ao, nxl, -1, s);
}

int FB_CAT(fbi_slab_x_pass_, FB_SUFFIX)(fb_plan* p, void* kslab, int nyl, int sign, hipStream_t s) {
    return launch_plain(p, p->N, slab_x(p, reinterpret_cast<cplx_t*>(kslab), nyl), nyl, sign, s);
}

int FB_CAT(fbi_slab_x_generate_, FB_SUFFIX)(fb_plan* p, void* kslab, int nyl, int ky0, uint64_t seed, uint64_t real,
                                            hipStream_t s) {
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.amp.shell = p->amp_shell.as<const real_t>();
    if (!op.amp.shell || p->amp_dense) { fb_set_error("slab generation needs shell amplitudes (cubic box)"); return FB_ERR_STATE; }
    op.amp.sym = p->amp_sym.as<const real_t>();
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    op.outer0 = ky0;
    return launch_strided<SMODE_GEN>(p, p->N, slab_x(p, reinterpret_cast<cplx_t*>(kslab), nyl), nyl, +1, op, s);
}

int FB_CAT(fbi_slab_x_bin_, FB_SUFFIX)(fb_plan* p, void* kslab, int nyl, int ky0, double* results, hipStream_t s) {
    if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    const int nb = p->nbins;
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.thr = p->thr; op.bins = p->bins; op.nbins = nb; op.namb = p->namb; op.store = 0; op.outer0 = ky0;
    for (int q = 0; q < 8; ++q) op.amb[q] = p->amb[q];
    int r = launch_strided<SMODE_BIN>(p, p->N, slab_x(p, reinterpret_cast<cplx_t*>(kslab), nyl), nyl, -1, op, s);
    if (r) return r;
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_sum_columns, dim3(2 * nb), dim3(256), 0, s, p->bin_partials, p->bin_rows, 2 * nb, results, (const double*)nullptr, 0LL, 0LL); }
    FB_LAUNCH_CHECK("k_sum_columns");
    return FB_OK;
}

// ---- the same passes over a RANGE of k_z tile columns (chunks): the all-to-all of one chunk runs beside the passes of
// the next.  A chunk of the k-space slab / of an exchange buffer lives in an array of its own with row pitch
// W = ntile * (columns per tile):  k-chunk [N][nyl][W],  exchange chunk [rank][nxl][nyl][W]  -- contiguous equal blocks
// per rank, as the collective needs them.  The x-slab's half spectrum [nxl][NR][NZP] keeps all columns in one array
// (the z pass reads whole rows), so the y passes have different row pitches on their two sides.
namespace {
constexpr int slab_tz(int N) {
    switch (N) {
        case 16: return tile_cols<real_t>(16); case 32: return tile_cols<real_t>(32); case 64: return tile_cols<real_t>(64);
        case 128: return tile_cols<real_t>(128); case 256: return tile_cols<real_t>(256); case 512: return tile_cols<real_t>(512);
        case 1024: return tile_cols<real_t>(1024); case 2048: return tile_cols<real_t>(2048);
    }
    return 0;
}
// blocked (exchange-buffer) side of a chunked y pass: pieces of a line are nxl*nyl*W apart
int slab_blocking_chunk(StridedArgs<real_t>& a, const fb_plan* p, int nxl, int nparts, long long W, bool out_side) {
    const int N = p->N, E = strided_elems(N);
    int m = E / nparts, shift = 0;
    if (nparts < 1 || m * nparts != E) { fb_set_error("fused slab exchange needs the rank count to divide the points per thread"); return FB_ERR_UNSUPPORTED; }
    while ((1 << shift) < m) ++shift;
    const long long nyl = N / nparts;
    a.blk_shift = shift;
    a.blk_stride = (long long)nxl * nyl * W;
    if (out_side) { a.blk_out = 1; a.out_stride = W; a.out_outer_stride = nyl * W; }
    else { a.blk_in = 1; a.out_stride = p->NZP; a.out_outer_stride = (long long)p->NR * p->NZP; a.stride = W; a.outer_stride = nyl * W; }
    return FB_OK;
}
}  // namespace

int FB_CAT(fbi_slab_tile_cols_, FB_SUFFIX)(const fb_plan* p) { return slab_tz(p->N); }

int FB_CAT(fbi_slab_x_generate_chunk_, FB_SUFFIX)(fb_plan* p, void* kchunk, int nyl, int ky0, uint64_t seed, uint64_t real,
                                                  int tile0, int ntile, hipStream_t s) {
    const int TZ = slab_tz(p->N);
    const long long W = (long long)ntile * TZ;
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.amp.shell = p->amp_shell.as<const real_t>();
    if (!op.amp.shell || p->amp_dense) { fb_set_error("slab generation needs shell amplitudes (cubic box)"); return FB_ERR_STATE; }
    op.amp.sym = p->amp_sym.as<const real_t>();
    op.key.k[0] = (uint32_t)seed; op.key.k[1] = (uint32_t)(seed >> 32);
    op.key.k[2] = (uint32_t)real; op.key.k[3] = (uint32_t)(real >> 32);
    op.outer0 = ky0;
    cplx_t* k = reinterpret_cast<cplx_t*>(kchunk) - (long long)tile0 * TZ;       // columns are addressed absolutely
    StridedArgs<real_t> a{k, k, p->tw.as<const cplx_t>(), (long long)nyl * W, W, p->NZV, (real_t)1};
    a.ntx = ntile; a.tile0 = tile0;
    return launch_strided<SMODE_GEN>(p, p->N, a, nyl, +1, op, s);
}

int FB_CAT(fbi_slab_y_inverse_chunk_, FB_SUFFIX)(fb_plan* p, const void* recv_chunk, void* half_local, int nxl, int nparts,
                                                 int tile0, int ntile, hipStream_t s) {
    const int TZ = slab_tz(p->N);
    const long long W = (long long)ntile * TZ;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    StridedArgs<real_t> a = slab_y(p, h);
    a.in = reinterpret_cast<const cplx_t*>(recv_chunk) - (long long)tile0 * TZ;
    int r = slab_blocking_chunk(a, p, nxl, nparts, W, false);
    if (r) return r;
    a.ntx = ntile; a.tile0 = tile0;
    return launch_plain(p, p->N, a, nxl, +1, s);
}

int FB_CAT(fbi_slab_y_forward_chunk_, FB_SUFFIX)(fb_plan* p, const void* half_local, void* send_chunk, int nxl, int nparts,
                                                 int tile0, int ntile, hipStream_t s) {
    const int TZ = slab_tz(p->N);
    const long long W = (long long)ntile * TZ;
    cplx_t* h = reinterpret_cast<cplx_t*>(const_cast<void*>(half_local));
    StridedArgs<real_t> a = slab_y(p, h);
    a.out = reinterpret_cast<cplx_t*>(send_chunk) - (long long)tile0 * TZ;
    int r = slab_blocking_chunk(a, p, nxl, nparts, W, true);
    if (r) return r;
    a.ntx = ntile; a.tile0 = tile0;
    return launch_plain(p, p->N, a, nxl, -1, s);
}

// the z passes of the x-slab on their own: 0 c2r (half -> real), 1 r2c (real -> half, optional exp), 2 c2r + r2c of
// (exp of) the same line (the field is written once and not read back)
int FB_CAT(fbi_slab_z_pass_, FB_SUFFIX)(fb_plan* p, void* half_local, void* real_local, int nxl, int which, double scale,
                                        int pre_exp, double* expsum, hipStream_t s) {
    const int N = p->N;
    cplx_t* h = reinterpret_cast<cplx_t*>(half_local);
    int r;
    if (which == 1) {
        ContigArgs<real_t> az{real_local, h, p->tw.as<const cplx_t>(), (long long)N, (long long)p->NZP, 0, N,
                              (long long)nxl * N, (real_t)1, pre_exp, nullptr, nullptr};
        r = launch_contig<ZMODE_R2C>(p, N / 2, az, -1, s);
    } else if (which == 2) {
        ContigArgs<real_t> az{h, real_local, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)N, N, 0,
                              (long long)nxl * N, (real_t)scale, pre_exp, nullptr, h};
        r = launch_contig<ZMODE_C2R2C>(p, N / 2, az, +1, s);
    } else {
        ContigArgs<real_t> az{h, real_local, p->tw.as<const cplx_t>(), (long long)p->NZP, (long long)N, N, 0,
                              (long long)nxl * N, (real_t)scale, 0, nullptr, nullptr};
        r = launch_contig<ZMODE_C2R>(p, N / 2, az, +1, s);
    }
    if (r) return r;
    if (which != 0 && pre_exp && expsum) {
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(1), dim3(256), 0, s, p->exp_partials, p->exp_rows, 1, expsum, (const double*)nullptr, 0LL, 0LL); }
        FB_LAUNCH_CHECK("k_sum_columns");
    }
    return FB_OK;
}

// x pass with the shell binning over one chunk; chunks are given in any order, `first` opens the shared table of
// partial sums (sized for every tile column of the slab), `last` sums it into results[2 nbins]
int FB_CAT(fbi_slab_x_bin_chunk_, FB_SUFFIX)(fb_plan* p, void* kchunk, int nyl, int ky0, int tile0, int ntile, int first,
                                             int last, double* results, hipStream_t s) {
    if (!p->nbins || !p->use_thr) { fb_set_error("fused P(k) needs shell thresholds (fb_set_bins with thr)"); return FB_ERR_STATE; }
    const int nb = p->nbins, TZ = slab_tz(p->N);
    const long long W = (long long)ntile * TZ;
    if (first) {
        const long long cap = (long long)((p->NZP + TZ - 1) / TZ) * nyl;      // one column per tile of the whole slab
        int r = p->bin_partials.ensure((size_t)cap * 2 * nb * sizeof(double));
        if (r) return r;
        p->bin_append_cols = cap;
        p->bin_rows = 0;
    }
    if (!p->bin_append_cols) { fb_set_error("fb_slab_x_bin_chunk: no chunk sequence open (first = 1)"); return FB_ERR_STATE; }
    StridedOp<real_t> op = {};
    op.g = fft_geom(p);
    op.thr = p->thr; op.bins = p->bins; op.nbins = nb; op.namb = p->namb; op.store = 0; op.outer0 = ky0;
    for (int q = 0; q < 8; ++q) op.amb[q] = p->amb[q];
    cplx_t* k = reinterpret_cast<cplx_t*>(kchunk) - (long long)tile0 * TZ;
    StridedArgs<real_t> a{k, k, p->tw.as<const cplx_t>(), (long long)nyl * W, W, p->NZV, (real_t)1};
    a.ntx = ntile; a.tile0 = tile0;
    int r = launch_strided<SMODE_BIN>(p, p->N, a, nyl, -1, op, s);
    if (r) { p->bin_append_cols = 0; return r; }
    if (last) {
        const long long rows = p->bin_rows, cap = p->bin_append_cols;
        p->bin_append_cols = 0;
        { FbProfScope _ps(p, FBK_BIN, s);
        hipLaunchKernelGGL(k_sum_columns, dim3(2 * nb), dim3(256), 0, s, p->bin_partials, rows, 2 * nb, results, (const double*)nullptr, 0LL, cap); }
        FB_LAUNCH_CHECK("k_sum_columns");
    }
    return FB_OK;
}

#ifdef FB_DEFINE_SLAB_PERMUTE
int fbi_slab_permute(fb_plan* p, const void* in, void* out, int nxl, int nparts, int pack, hipStream_t s) {
    const int N = p->N, nyl = N / nparts;
    const int row_vec = p->NZP * 2 * p->prec / 16;          // 16-byte vectors per row
    dim3 grid((row_vec + 63) / 64, N, nxl);
    { FbProfScope _ps(p, FBK_LAYOUT, s);
    if (pack) hipLaunchKernelGGL(k_slab_permute<1>, grid, dim3(64), 0, s, (const uint4*)in, (uint4*)out, nxl, nyl, nparts, row_vec, p->NR);
    else      hipLaunchKernelGGL(k_slab_permute<0>, grid, dim3(64), 0, s, (const uint4*)in, (uint4*)out, nxl, nyl, nparts, row_vec, p->NR); }
    FB_LAUNCH_CHECK("k_slab_permute");
    return FB_OK;
}
#endif
