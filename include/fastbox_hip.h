/*
 * libfastbox_hip -- C ABI of the MI355X (gfx950) density-field hot path.
 *
 * The reference (philbull/FastBox, fastbox/box.py) has no FFI layer: its hot
 * path is numpy calls inside the methods of `CosmoBox`.  This header is the
 * boundary a ctypes/cffi binding of those methods binds instead; every entry
 * point names the reference lines whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a
 *     negative FB_ERR_* code, and fb_last_error() (thread local) says why;
 *   - all field pointers are DEVICE pointers owned by the caller (hipMalloc,
 *     a torch tensor's data_ptr(), ...).  `stream` is a hipStream_t (NULL =
 *     default stream); calls are asynchronous unless stated otherwise;
 *   - precision is fixed per plan: 4 = float / complex64, 8 = double /
 *     complex128 (the reference is float64 throughout);
 *   - layouts are C order with z fastest, like the reference's ndarrays:
 *       real : T          [N][N][N]
 *       full : complex<T> [N][N][N]
 *       half : complex<T> [N][rows][pitch], k_z = 0..N/2 stored, pitch = fb_half_pitch(),
 *              rows = fb_half_rows() = N + 1 of which the first N are used (the spare row keeps
 *              the x stride off a multiple of 64 KiB; size the buffer with fb_half_bytes())
 *     A half spectrum represents the Hermitian array fftn(real field).
 *   - one plan per host thread at a time (thread compatible, not thread safe).
 */
#ifndef FASTBOX_HIP_H
#define FASTBOX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK 0
#define FB_ERR_INVALID -1      /* bad argument                        */
#define FB_ERR_HIP -2          /* HIP runtime / launch failure        */
#define FB_ERR_UNSUPPORTED -3  /* grid size not a power of two 16..2048 */
#define FB_ERR_NOMEM -4
#define FB_ERR_STATE -5        /* tables not set before use           */
#define FB_ERR_RCCL -6         /* RCCL missing or a collective failed (fb_comm_*, fb_slab_exchange*, fb_allreduce_f64) */

typedef struct fb_plan fb_plan;

int fb_version(void);
const char* fb_last_error(void);

/* ---- plan: geometry of one CosmoBox (box.py:25-127) ---------------------------------- */
/* axis2[3*N]: (m_i/L_a)**2; ksc[3*N]: m_i*(2 pi/L_a); kpar[N]: 2 pi m_i/Lz; zgrid[N]: self.z.
 * They are computed by the host binding with the reference's numpy expressions
 * (box.py:119-127, 254-256, 375, 79-88) so that |k| is bit-identical.            */
/* N: a power of two in 16 .. 2048 (the tuned kernels, every entry point), or any other EVEN size with prime factors 2, 3, 5 in
 * 16 .. 1024 (round 4): there fb_fft_c2c / _r2c / _c2r run plain Stockham passes (radices 4, 2, 3, 5) and every kernel that is not
 * an FFT pass works as usual (the transverse and 2-D transforms behind fb_fft_transverse, fb_beam_convolve, fb_sky_realise_map take
 * the same plain passes), while the entry points that fuse something into an FFT pass (fb_realise_density_*,
 * fb_power_spectrum_*, fb_slab_*) return FB_ERR_UNSUPPORTED: compose
 * fb_colour_device / fb_colour_noise + fb_fft_c2r, fb_fft_r2c + fb_bin_power, fb_lognormal ... instead, as
 * fastbox_amd.CosmoBox does on such a grid.  Anything else (odd, other prime factors): FB_ERR_UNSUPPORTED. */
int fb_plan_create(fb_plan** plan, int N, double Lx, double Ly, double Lz, int precision, int device,
                   const double* axis2, const double* ksc, const double* kpar, const double* zgrid);
int fb_plan_destroy(fb_plan* plan);
int fb_half_pitch(const fb_plan* plan);          /* complex elements per (x,y) row of a half spectrum */
int fb_half_rows(const fb_plan* plan);           /* stored rows per x-plane of a half spectrum (N + 1)   */
int64_t fb_real_bytes(const fb_plan* plan);
int64_t fb_half_bytes(const fb_plan* plan);
int64_t fb_full_bytes(const fb_plan* plan);

/* ---- 3-D FFTs (numpy.fft.fftn / ifftn, box.py:187,193,246,337,380,654,736) ------------- */
/* in place on a full complex array; direction -1 = fftn, +1 = ifftn (scale applied: pass 1/N^3) */
int fb_fft_c2c(fb_plan* plan, void* full_inout, int direction, double scale, void* stream);
/* fftn of a real field -> half spectrum.  pre_exp != 0 transforms exp(field) (log-normal fusion) */
int fb_fft_r2c(fb_plan* plan, const void* real_in, void* half_out, int pre_exp, void* stream);
/* Re ifftn of the Hermitian array a half spectrum stands for; `half_inout` is destroyed */
int fb_fft_c2r(fb_plan* plan, void* half_inout, void* real_out, double scale, void* stream);

/* ---- Gaussian realisation (realise_density, box.py:161-187) --------------------------- */
/* sqrt(nan_to_num(P(k)) * boxfactor): per integer shell n^2=i^2+j^2+l^2 (cubic boxes) ...   */
int fb_set_amplitude_shells(fb_plan* plan, const double* amp, int64_t nshell);
/* ... or, for any box shape, per (|m_x|, |m_y|, |m_z|): HOST double[M][M][M], M = N/2 + 1 (|k| depends on the mode
 * numbers only through their magnitudes: an eighth of the modes to evaluate P(k) on) ...                     */
int fb_set_amplitude_sym(fb_plan* plan, const double* amp, int64_t n);
/* ... or per stored mode, a DEVICE array T[N][rows][pitch] (any box shape)                 */
int fb_set_amplitude_dense(fb_plan* plan, const void* amp_dev);
/* parity mode: re, im are the reference's np.random.normal draws, T[N][N][N] on the device  */
int fb_colour_noise(fb_plan* plan, const void* re, const void* im, void* half_out, void* stream);
/* throughput mode: Philox4x32-10, key = seed, counter = (mode index, stream, realisation); fb_rng.h */
int fb_colour_device(fb_plan* plan, uint64_t seed, uint64_t realisation, void* half_out, void* stream);

/* fused throughput path: generator inside the first inverse pass, then y and z (c2r) passes.
 * real_out = Re ifftn(X)/1 with numpy's 1/N^3; work_half is scratch (half-spectrum sized).  */
int fb_realise_density_device(fb_plan* plan, uint64_t seed, uint64_t realisation, void* work_half,
                              void* real_out, void* stream);

/* velocity component `comp` (0 x, 1 y, 2 z) of the SAME realisation in real space:
 * real_out = Re ifftn(i fac delta_k k_c / k^2) (realise_velocity, box.py:251-284, then the caller's
 * np.fft.ifftn(velocity_k[c]).real, e.g. examples/example_redshift_space.py:17).  The counter-based
 * generator reproduces delta_k inside the first pass; no spectrum is stored.  work_half is scratch. */
int fb_realise_velocity_device(fb_plan* plan, uint64_t seed, uint64_t realisation, int comp, double fac,
                               void* work_half, void* real_out, void* stream);

/* deferred form of the above: _begin runs the generator + x pass into `pending_half` (half-spectrum
 * sized); the y and z passes are done later by _finish (real_out = delta_x), or by
 * fb_power_spectrum_pending, which fuses the z pass with the first pass of the power spectrum:
 * real_out is written (delta_x is still produced) but never read back.  The y and z passes of every
 * transform run x-plane batch by x-plane batch, so that a batch stays in the Infinity Cache between
 * them (env FB_PLANE_BATCH = planes per batch, 0 = off; FB_PLANE_STREAMS = 1 | 2: with 2, the default
 * from 1024^3 up, alternate batches run on a plan-owned auxiliary stream that is joined back into
 * `stream` before the call returns).                                                            */
int fb_realise_density_begin(fb_plan* plan, uint64_t seed, uint64_t realisation, void* pending_half, void* stream);
int fb_realise_density_finish(fb_plan* plan, void* pending_half, void* real_out, void* stream);

/* ---- binned power spectrum (binned_power_spectrum, box.py:741-764) ------------------------- */
/* edges[nbins] as in np.digitize(k, edges).  thr/amb describe, for cubic boxes, the bin as a
 * step function of the integer shell (thr[b] = first n^2 with |k| >= edges[b]; amb = shells
 * to decide with the exact fp64 |k|); pass thr = NULL to always use the exact expression.   */
int fb_set_bins(fb_plan* plan, const double* edges, int nbins, const int32_t* thr, const int32_t* amb, int namb);
/* spec: layout 1 = half spectrum (mirrored modes counted twice), 0 = full complex array.
 * host outputs: count[nbins] (modes of the full grid per bin), sum[nbins] = sum |dk|^2,
 * sumsq[nbins] = sum |dk|^4.  Synchronises the stream.                                       */
int fb_bin_power(fb_plan* plan, const void* spec, int layout, double* count, double* sum, double* sumsq,
                 void* stream);
/* the same sums of spec * T(k_perp, k_par) (filter kinds and params as fb_apply_filter): the power
 * spectrum of apply_transfer_fn's result (box.py:356-381 then :741-764) for a real, k_par-even filter,
 * without storing the filtered spectrum or transforming back and forth.                      */
int fb_bin_power_filtered(fb_plan* plan, const void* spec, int layout, int kind, const double* params,
                          const void* table_dev, double* count, double* sum, double* sumsq, void* stream);

/* fused "filter + estimate" for cubic boxes (needs fb_set_bins with thr): the power spectrum of
 * ifftn(fftn(real_in) * T(k_perp, k_par)) for a real, k_par-even filter -- apply_transfer_fn followed by
 * binned_power_spectrum (box.py:356-381, :696-768).  r2c and y pass, then the x pass multiplies by T,
 * writes the FILTERED spectrum to filtered_half (fb_fft_c2r of it delivers the filtered field) and bins
 * it.  kind: FB_FILT_TABLE, FB_FILT_BEAM_HIGHPASS or FB_FILT_WEDGE (FB_FILT_TOPHAT, smooth_field's window, is
 * applied with fb_apply_filter: FB_ERR_UNSUPPORTED here).  Asynchronous; results_dev as for fb_power_spectrum_device. */
int fb_power_spectrum_filtered(fb_plan* plan, const void* real_in, void* filtered_half, int kind,
                               const double* params, const void* table_dev, void* results_dev, void* stream);
/* the same when what the caller goes on to read is the filtered FIELD (apply_transfer_fn's return value,
 * box.py:381): the x pass that filters and bins a line also takes the line's inverse transform, so work_half
 * receives the filtered spectrum already transformed back along x and fb_fft_c2r_yz (the y and z passes of
 * fb_fft_c2r; work_half is destroyed) delivers the field -- one read and one write of the spectrum fewer.   */
int fb_power_spectrum_filtered_field(fb_plan* plan, const void* real_in, void* work_half, int kind,
                                     const double* params, const void* table_dev, void* results_dev, void* stream);
int fb_fft_c2r_yz(fb_plan* plan, void* half_x_done, void* real_out, double scale, void* stream);

/* BASELINE configs[2] as one chain (examples/example_redshift_space.py: realise_density, realise_velocity, box.py:384-438
 * redshift_space_density, then np.fft.fftn of the result and box.py:356-381 / :696-768 on it), for a device-generator
 * realisation.  fb_realise_velocity_begin: generator + first inverse pass of velocity component comp (fac = box.py:280-281),
 * deferred like fb_realise_density_begin (fb_realise_density_finish delivers the component in real space).
 * fb_power_spectrum_redshift_space: pending_delta / pending_vz (both destroyed) -> delta_x_out (the density in real space;
 * NULL: not written), the P(k) sums of the redshift-space field in results_dev (as fb_power_spectrum_device), and, when
 * filter_kind >= 0 (FB_FILT_TABLE, _BEAM_HIGHPASS, _WEDGE as fb_power_spectrum_filtered; -1: no filter, work_half is
 * scratch), the filtered spectrum in work_half -- want_field: already transformed back along x, for fb_fft_c2r_yz.
 * The two inverse z passes, the line-of-sight remap and the forward z pass are ONE kernel per plane batch: v_z in real
 * space and the redshift-space field itself never reach memory (4 half-sweeps of traffic instead of 9).  The numbers are
 * those of fb_realise_density_finish + fb_realise_velocity_device + fb_redshift_space + fb_power_spectrum_filtered[_field],
 * bit for bit.  Hz, sigma_nl, seed, method: as fb_redshift_space (sigma_nl > 0 draws the device noise of that call).
 * Single-precision plans with 64 <= N <= 512 (FB_ERR_UNSUPPORTED otherwise: use the separate calls).                  */
int fb_realise_velocity_begin(fb_plan* plan, uint64_t seed, uint64_t realisation, int comp, double fac,
                              void* pending_half, void* stream);
int fb_power_spectrum_redshift_space(fb_plan* plan, void* pending_delta, void* pending_vz, void* delta_x_out,
                                     void* work_half, double Hz, double sigma_nl, uint64_t seed, int method,
                                     int filter_kind, const double* params, const void* table_dev, int want_field,
                                     void* results_dev, void* stream);

/* fused path for cubic boxes (needs fb_set_bins with thr): r2c of real_in (of exp(real_in) when
 * pre_exp) with the binning inside the last pass.  Asynchronous: results_dev[2*nbins+1] (DEVICE)
 * receives (sum |dk|^2, sum |dk|^4) per bin, then sum(exp(real_in)) (0 unless pre_exp).
 * work_half is scratch and holds fftn(real_in) afterwards only if keep_spectrum.              */
int fb_power_spectrum_device(fb_plan* plan, const void* real_in, void* work_half, int pre_exp,
                             int keep_spectrum, double* results_dev, void* stream);
/* same results for a field still pending from fb_realise_density_begin (see there); consumes pending_half.
 * real_out = NULL: delta_x itself is not written (a Monte-Carlo loop that only wants the spectrum; the realisation can
 * be regenerated from (seed, realisation) at any time) -- a quarter of the fused z pass's traffic less.            */
int fb_power_spectrum_pending(fb_plan* plan, void* pending_half, void* real_out, int pre_exp, double* results_dev,
                              void* stream);
/* A Monte-Carlo loop in one call: for i < count, realisation (seed, first + i stride) is drawn (fb_realise_density_begin into
 * work_half) and its P(k) estimated (fb_power_spectrum_pending; real_out, if given, receives every field in turn and holds
 * the last one), results_dev[i * results_stride ...] = the 2 nbins + 1 sums of realisation i.  The same launches in the same
 * order as the two calls per realisation -- identical numbers -- without an interpreter between them: what a step of a box
 * below 256^3 is bound by.  Needs the amplitude table and fb_set_bins with thr, like the calls it stands for.               */
int fb_montecarlo_power(fb_plan* plan, uint64_t seed, uint64_t first, uint64_t stride, int count, void* work_half, void* real_out,
                        int pre_exp, double* results_dev, int64_t results_stride, void* stream);
/* number of full-grid modes per bin for the current bin set (host array, nbins doubles) */
int fb_bin_counts(fb_plan* plan, double* count);

/* ---- two-point correlation function ------------------------------------------------------------------------ */
/* What the reference's examples end with, through nbodykit: examples/example_corr_fn.py:38-47
 * (FFTCorr(first=mesh, mode='1d', los=[0,0,1], dr=2., rmin=10., rmax=200.) of delta_x and of lognormal(delta_x)), and step
 * (6) of examples/End-to-end_simulation.ipynb / "Example end-to-end analysis.ipynb" (the same call on the true and on the
 * PCA-cleaned cube, dr=2., rmin=20., rmax=200.).  Definition, for real fields d_1, d_2 (auto: d_2 = d_1):
 *   D_a = fftn(d_a - mean(d_a)),  xi(s) = ifftn(conj(D_1) D_2) / N^3 = (1/N^3) sum_x d_1(x) d_2(x + s)  (periodic);
 *   s_a = m_a (L_a / N), m_a the signed index (Nyquist negative); |s| = sqrt((s_x s_x + s_y s_y) + s_z s_z) in fp64,
 *   no contraction; mu = s_z / |s| (0 at s = 0; the line of sight is z); bin b = [edges[b], edges[b+1]), i.e.
 *   np.digitize(|s|, edges) - 1, separations outside [edges[0], edges[nbins]) dropped.
 * Nothing is fused into an FFT pass: every grid a plan accepts.
 * fb_cross_power_half: half_out = conj(half1) half2 * scale on half spectra (half2 = NULL: |half1|^2, imaginary part 0), the
 *   k = 0 mode set to 0 (the mean removed).  half_out may be half1 or half2.  fb_fft_c2r applies exactly the scale it is given
 *   (no implicit 1/N^3): scale = 1/N^6 here and 1 there deliver xi.
 * fb_bin_separation: per-bin sums over the separations of a real field xi; edges[nbins + 1] strictly ascending, edges[0] >= 0,
 *   1 <= nbins <= 1024, lmax 0, 2 or 4 (FB_ERR_INVALID otherwise).  out_host[(2 + lmax/2 + 1) nbins] = npairs[nbins] (cells per
 *   bin), sum_r[nbins] (sum |s|), then sum[lmax/2 + 1][nbins] = sum xi(s) L_l(mu), l = 0, 2, ..  (xi_l = (2l + 1) sum / npairs;
 *   nbodykit's r column = sum_r / npairs).  npairs and sum_r do not depend on the data: computed once per bin set and kept in the
 *   plan.  Synchronises the stream.
 * fb_correlation_function: the whole chain -- fb_fft_r2c of real1 (and real2, NULL: auto-correlation) into work_half1
 *   (work_half2), fb_cross_power_half, fb_fft_c2r into work_real (which then holds xi), fb_bin_separation.  Synchronises. */
int fb_cross_power_half(fb_plan* plan, const void* half1, const void* half2, void* half_out, double scale, void* stream);
int fb_bin_separation(fb_plan* plan, const void* real, const double* edges, int nbins, int lmax, double* out_host,
                      void* stream);
int fb_correlation_function(fb_plan* plan, const void* real1, const void* real2, void* work_half1, void* work_half2,
                            void* work_real, const double* edges, int nbins, int lmax, double* out_host, void* stream);

/* ---- power spectrum in (k, mu) bins, cross spectra, multipoles ----------------------------------------------- */
/* What the reference's examples take from nbodykit as FFTPower(first=, second=, mode='1d' | '2d', los=[0,0,1], Nmu=, dk=,
 * kmin=, kmax=, poles=) (examples/example_box.py:48-52, examples/example_halos.py:46-52).  Definition, for real fields d_1,
 * d_2 (auto: d_2 = d_1):
 *   D_a = rfftn(d_a) (unnormalised); P(k) = (Lx Ly Lz / N^6) Re(conj(D_1(k)) D_2(k)), products and sums in fp64;
 *   k_a = m_a (2 pi / L_a), m_a the signed index (Nyquist negative); |k| = sqrt((k_x k_x + k_y k_y) + k_z k_z) in fp64, no
 *   contraction; mu = |k_z| / |k| (line of sight z).  Modes of the full grid: a half-spectrum cell with 0 < m_z < N/2 counts
 *   twice, the planes m_z = 0 and N/2 once; k = 0 is excluded.  k bin b = [kedges[b], kedges[b+1]) = np.digitize(|k|,
 *   kedges) - 1, modes outside [kedges[0], kedges[nk]) dropped; mu bin c = np.digitize(mu, np.linspace(0, 1, nmu + 1)) - 1
 *   with mu >= 1 in the last bin.  Cell (b, c) has index b nmu + c.
 * Limits (FB_ERR_INVALID otherwise): kedges[nk + 1] strictly ascending, kedges[0] >= 0, all finite but the last (which may be
 *   inf); 1 <= nk <= 1024; 1 <= nmu <= 128; lmax 0, 2 or 4; nk nmu (lmax/2 + 1) <= 5120 (one wave's LDS row: 1024 k bins x 5 mu
 *   bins, or 1024 x 1 with lmax 4).
 * fb_bin_power_kmu: bins Re(conj(half1) half2) (half2 = NULL: |half1|^2) straight from the stored half spectra, without
 *   writing the product.  out_host[4 nk nmu + (lmax/2) nk] (nc = nk nmu):
 *     modes[nc] (full-grid modes per cell), sum_k[nc] (sum |k|), sum_mu[nc] (sum mu), sum_p[nc] (sum P),
 *     then sum P L_l over each k bin's mu cells [nk] for l = 2, 4 up to lmax.
 *   nbodykit's columns are k = sum_k / modes, mu = sum_mu / modes, power = sum_p / modes, and the multipoles
 *   P_l = (2l + 1) sum P L_l / modes of the 1-d bin.  modes, sum_k and sum_mu do not depend on the data: computed once per
 *   (kedges, nmu) and kept in the plan.  Synchronises the stream.
 * fb_power_spectrum_kmu: fb_fft_r2c of real1 (and real2; NULL: auto spectrum) into work_half1 (work_half2), then
 *   fb_bin_power_kmu.  Every grid a plan accepts.  Synchronises. */
int fb_bin_power_kmu(fb_plan* plan, const void* half1, const void* half2, const double* kedges, int nk, int nmu, int lmax,
                     double* out_host, void* stream);
int fb_power_spectrum_kmu(fb_plan* plan, const void* real1, const void* real2, void* work_half1, void* work_half2,
                          const double* kedges, int nk, int nmu, int lmax, double* out_host, void* stream);

/* ---- cylindrical power P(k_perp, k_par) and multi-frequency angular power C(k_perp; nu, nu') ------------------------- */
/* Two estimators that bin the transverse modes (m_x, m_y) in k_perp and keep the line of sight (z, the frequency axis)
 * resolved.  The reference and nbodykit have neither: these definitions are the contract.  Conventions are those of
 * fb_bin_power_kmu: k_a = m_a (2 pi / L_a), m_a the signed index (Nyquist negative); k_perp = sqrt(k_x k_x + k_y k_y) in fp64,
 * no contraction; k_perp bin b = np.digitize(k_perp, perp_edges) - 1, modes outside [perp_edges[0], perp_edges[n]) dropped;
 * products and sums in fp64 in a fixed order without atomics (two calls agree bit for bit).
 *
 * Cylindrical power, for real fields d_1, d_2 (auto: d_2 = d_1):
 *   D_a = rfftn(d_a) (unnormalised); P(k) = (Lx Ly Lz / N^6) Re(conj(D_1(k)) D_2(k)); k_par = |k_z|; k_par bin
 *   c = np.digitize(k_par, par_edges) - 1.  Modes of the full grid: a half-spectrum cell with 0 < m_z < N/2 counts twice, the
 *   planes m_z = 0 and N/2 once; k = 0 is excluded.  Cell (b, c) has index b npar + c.
 * Limits (FB_ERR_INVALID otherwise): perp_edges[nperp + 1] strictly ascending, perp_edges[0] >= 0, all finite but the last
 *   (which may be inf); par_edges[npar + 1] strictly ascending, all finite but the last (the first may be negative: the
 *   default edges put one bin around every |m_z|); 1 <= nperp <= 1024; 1 <= npar <= 1025.
 * fb_bin_power_cyl: bins Re(conj(half1) half2) (half2 = NULL: |half1|^2) straight from the stored half spectra.
 *   out_host[4 nperp npar] (nc = nperp npar): modes[nc], sum_kperp[nc], sum_kpar[nc], sum_p[nc]; the columns of a cell are
 *   kperp = sum_kperp / modes, kpar = sum_kpar / modes, power = sum_p / modes.  The transverse rows sorted by k_perp bin are
 *   built once per perp_edges and kept in the plan (the eight most recent edge sets).  Synchronises the stream.
 * fb_power_spectrum_cyl: fb_fft_r2c of real1 (and real2; NULL: auto spectrum) into work_half1 (work_half2), then
 *   fb_bin_power_cyl.  Every grid a plan accepts.  Synchronises.
 *
 * Multi-frequency angular power (the flat-sky C_l(nu, nu') of Datta et al. 2007, Mondal et al. 2018), for real cubes d_1, d_2:
 *   a_a(m_perp, nu) = np.fft.fftn(d_a, axes=(0, 1)) (unnormalised), every m_perp of the full N x N plane but m_perp = 0;
 *   C_b(nu, nu') = (Lx Ly / N^4) (1 / modes_b) sum_{m_perp in b} Re(a_1(m_perp, nu) conj(a_2(m_perp, nu'))).
 *   The first channel index belongs to cube 1, the second to cube 2; the auto result is symmetric bit for bit.  An empty bin
 *   is NaN.  The operands are held in the plan's precision and converted to fp64 on load; the sums run on the fp64 matrix cores.
 * Limits (FB_ERR_INVALID otherwise): perp_edges as above; 1 <= nb <= 256; N <= 1024.
 * fb_transverse_gram: full1, full2 (NULL: auto) are complex [N][N][N] cubes already transformed by fb_fft_transverse(-1).
 *   cl_dev[nb][N][N] (device, fp64) receives C_b; work_dev: fb_transverse_gram_work_bytes(plan, nb, cross) bytes of device
 *   memory for the per-(bin, slice) partials; out_host[2 nb]: modes[nb], sum_kperp[nb].  Synchronises.
 * fb_angular_power: fb_real_to_complex and fb_fft_transverse(-1) of real1 into work_full1 (and of real2, if given, into
 *   work_full2), then fb_transverse_gram.  Synchronises. */
int fb_bin_power_cyl(fb_plan* plan, const void* half1, const void* half2, const double* perp_edges, int nperp,
                     const double* par_edges, int npar, double* out_host, void* stream);
int fb_power_spectrum_cyl(fb_plan* plan, const void* real1, const void* real2, void* work_half1, void* work_half2,
                          const double* perp_edges, int nperp, const double* par_edges, int npar, double* out_host,
                          void* stream);
long long fb_transverse_gram_work_bytes(const fb_plan* plan, int nb, int cross);
int fb_transverse_gram(fb_plan* plan, const void* full1, const void* full2, const double* perp_edges, int nb, double* cl_dev,
                       void* work_dev, double* out_host, void* stream);
int fb_angular_power(fb_plan* plan, const void* real1, const void* real2, void* work_full1, void* work_full2,
                     const double* perp_edges, int nb, double* cl_dev, void* work_dev, double* out_host, void* stream);

/* ---- bispectrum in triangle bins ----------------------------------------------------------------------------------- */
/* The FFT estimator of the bispectrum of a real field d (Scoccimarro 2000; Sefusatti et al. 2016) in bins of three |k| shells.
 * The reference and nbodykit have none: this definition is the contract.  It follows the conventions of fb_bin_power_kmu:
 *   D = fftn(d) (unnormalised; the mean is not subtracted, k = 0 never enters); k_a = m_a (2 pi / L_a), m_a the signed index
 *   (Nyquist negative); |k| = sqrt((k_x k_x + k_y k_y) + k_z k_z) in fp64, no contraction;
 *   shell S_b = {m != 0 of the full grid : np.digitize(|k|, kedges) - 1 == b}, b = 0 .. nb - 1;
 *   I_b(x) = sum_{m in S_b} D(m) exp(+2 pi i m.x / N) (real: S_b is symmetric under m -> -m mod N); U_b the same with D = 1;
 *   for every triple t = (b1 <= b2 <= b3), in itertools.combinations_with_replacement(range(nb), 3) order,
 *     ntri_t = sum_x U_b1 U_b2 U_b3 / N^3 = #{(m1, m2, m3) in S_b1 x S_b2 x S_b3 : m1 + m2 + m3 = 0 (mod N, per axis)},
 *     B_t = (V^2 / N^12) sum_x I_b1 I_b2 I_b3 / ntri_t,  V = Lx Ly Lz.
 *   Triangles close modulo N: with kedges[nb] <= (2/3) pi N / max(L) none closes through an alias.  The cubes I_b are held in
 *   the plan's precision; their products and sums over x are fp64 on the matrix cores, in a fixed order (two calls agree bit
 *   for bit).
 * Limits (FB_ERR_INVALID otherwise): kedges[nb + 1] strictly ascending, kedges[0] >= 0, all finite but the last; 1 <= nb <= 32;
 *   1 <= nwork <= 4; N <= 1024.
 * fb_bispectrum: fb_fft_r2c of `real` into work_half; then, nwork shells per read of it, the spectrum is split into
 *   work_shells (nwork half spectra, destroyed) and each shell goes through fb_fft_c2r into its cube of `cubes` (nb real
 *   fields, which hold the I_b afterwards); one sweep over the voxels then forms every triple's sum.  unit != 0: D = 1 on every
 *   mode (real and work_half are not used and may be NULL), i.e. the U_b and N^3 ntri_t -- data-independent, so callers keep
 *   it per edge set, and form it on a double-precision plan.  out_host[T + 3 nb], T = nb (nb + 1) (nb + 2) / 6:
 *     sum[T] (sum_x I_b1 I_b2 I_b3), then per shell modes[nb] (|S_b|), sum_k[nb] (sum |k|), sum_p[nb] (sum |D|^2); cells of
 *   the half spectrum with 0 < m_z < N/2 count twice.  P_b = (V / N^6) sum_p / modes is the shell's power, the reduced
 *   bispectrum Q_t = B_t / (P_b1 P_b2 + P_b2 P_b3 + P_b3 P_b1).  Every grid a plan accepts up to 1024^3.  Synchronises.
 * fb_device_memory: free and total bytes of the calling thread's current device (hipMemGetInfo). */
int fb_bispectrum(fb_plan* plan, const void* real, void* work_half, void* work_shells, int nwork, void* cubes,
                  const double* kedges, int nb, int unit, double* out_host, void* stream);
int fb_device_memory(int64_t* free_bytes, int64_t* total_bytes);

/* ---- halo tracers (fastbox/halos.py, examples/example_halos.py) --------------------------------------------------- */
/* fb_halo_lambda: the expected count per voxel, lam_out (DEVICE double[N^3]), exactly halo_count_field's expression
 * (halos.py:92-114) in fp64 whatever the plan's precision:
 *   delta_h = bias * delta;  log-normal: delta_h = exp(delta_h - s) / mean(exp(delta_h - s)) - 1 (s = 0 on fp64 plans, the
 *   field's maximum of bias * delta on fp32 plans; mean = sum / N^3);  lam = (voxel_vol * nbar) * (1 + delta_h), each
 *   operation rounded once (no contraction);  lam < 0 -> 0 unless log-normal;  NaN -> 0.
 * nbar, bias: kind FB_HALO_SCALAR (value `*_val`, pointer unused), FB_HALO_ZPROFILE (DEVICE double[N], indexed by z),
 * FB_HALO_FIELD (DEVICE field of the plan's precision), FB_HALO_FIELD_F64 (DEVICE double[N^3]).  voxel_vol = Lx Ly Lz / N^3.
 * fb_halo_counts: the same lam, then a Poisson draw per voxel into counts_out (real field of the plan's precision holding
 *   integers): inversion of the CDF with one uniform per voxel, u = (w + 1/2) 2^-53 with w = (o0 << 21) | (o1 >> 11) the
 *   words of Philox call `voxel` of stream 5 (fb_rng.h), in fp64.  *too_large = 1 if some lam > 2^24 (those voxels get 0).
 *   Synchronises the stream.                                                                                              */
#define FB_HALO_SCALAR 0
#define FB_HALO_ZPROFILE 1
#define FB_HALO_FIELD 2
#define FB_HALO_FIELD_F64 3
int fb_halo_lambda(fb_plan* plan, const void* delta, const void* nbar, int nbar_kind, double nbar_val, const void* bias,
                   int bias_kind, double bias_val, double voxel_vol, int lognormal, double* lam_out, void* stream);
int fb_halo_counts(fb_plan* plan, const void* delta, const void* nbar, int nbar_kind, double nbar_val, const void* bias,
                   int bias_kind, double bias_val, double voxel_vol, int lognormal, uint64_t seed, uint64_t realisation,
                   void* counts_out, int* too_large, void* stream);
/* Halo catalogue (realise_halo_catalogue, halos.py:120-176) of a counts field (real field of the plan's precision, non-negative
 * integers).  fb_halo_catalogue_size: kmax_total[0] = the largest count, [1] = the number of halos (FB_ERR_INVALID if a value
 * is negative, not an integer or not finite); synchronises.  fb_halo_catalogue: pos_out (DEVICE double[total][3]) in the
 * reference's order -- ascending count; within a count, voxels in C order, each repeated `count` times -- with
 * pos[h][a] = (i_a + u) * (L_a / N), two fp64 operations.  scatter 0: u = 0; 1: u = uniforms[3 h + a] (DEVICE double[3 total]);
 * 2: u = (1 - 1e-8) * (o_a 2^-32), o_a the words of Philox call h of stream 6.  Asynchronous (plan-owned work tables).          */
int fb_halo_catalogue_size(fb_plan* plan, const void* counts, int64_t* kmax_total, void* stream);
int fb_halo_catalogue(fb_plan* plan, const void* counts, int64_t kmax, int64_t total, const double* uniforms, int scatter,
                      uint64_t seed, uint64_t realisation, double* pos_out, void* stream);
/* Mass assignment (nbodykit's to_mesh, examples/example_halos.py): real_out = sum over particles of weight * W, periodic.
 * pos: DEVICE double[n][3]; weights: DEVICE double[n] or NULL (all 1).  Node m sits at m L_a / N, u = x N / L_a:
 *   NGP: node floor(u + 1/2);  CIC: floor(u), floor(u) + 1 with 1 - f, f (f = u - floor(u));
 *   TSC: floor(u + 1/2) + (-1, 0, 1) with 1/2 (1/2 - d)^2, 3/4 - d^2, 1/2 (1/2 + d)^2 (d = u - floor(u + 1/2)).
 * Accumulated in fixed point (int64; two words on fp64 plans): the result does not depend on the order of the adds and is
 * the same bit for bit from call to call.  At most 2^31 contributions per node.  Asynchronous.
 * fb_paint_compensate: real_inout = ifftn(fftn(real_inout) / prod_a sinc(pi m_a / N)^p), p = window + 1 (1 NGP, 2 CIC,
 *   3 TSC), m_a the signed FFT index; work_half is scratch (half-spectrum sized).                                         */
#define FB_WINDOW_NGP 0
#define FB_WINDOW_CIC 1
#define FB_WINDOW_TSC 2
int fb_paint(fb_plan* plan, const double* pos, const double* weights, int64_t n, int window, void* real_out, void* stream);
int fb_paint_compensate(fb_plan* plan, void* real_inout, void* work_half, int window, void* stream);

/* ---- COLA particle mesh (realise_density_cola, box.py:463-589; definition in DESIGN.md section 4) ---------------------------
 * Cubic, single-GPU plans, N^3 particles.  Particle i starts on node i (C order) at q = m L / N, so "per-particle" arrays are
 * real fields of the plan's precision: psi1, psi2, pres, force are [3][N^3] blocks (component-major, indexed by particle);
 * positions are DEVICE double[N^3][3] in Mpc, wrapped to [0, L).  k_a = 2 pi m_a / L with m_a the signed FFT index
 * (fftfreq: N/2 -> -N/2).  Every transform is fb_fft_r2c / fb_fft_c2r with scale 1/N^3; work_half1/2 are half-spectrum sized.
 * Asynchronous.
 * fb_cola_lpt: from delta0 (real, z = 0 linear density): psi1 = c2r(i k delta0(k) / k^2); the six phi_ab = c2r(k_a k_b
 *   delta0(k) / k^2); S = phi_xx phi_yy + phi_xx phi_zz + phi_yy phi_zz - phi_xy^2 - phi_xz^2 - phi_yz^2 (one pass);
 *   psi2 = c2r(-i k S(k) / k^2).  k = 0 is zeroed; i k_a and k_a k_b (a != b) are zeroed on the planes m_a = -N/2 (and
 *   m_b = -N/2); k_a^2 is not.  work3: [3][N^3] real scratch.                                                               */
int fb_cola_lpt(fb_plan* plan, const void* delta0, void* psi1, void* psi2, void* work3, void* work_half1, void* work_half2,
                void* stream);
/* fb_cola_init: pos = wrap(q + d1 psi1 + d2 psi2); pres = 0 (pres may be NULL).                                               */
int fb_cola_init(fb_plan* plan, const void* psi1, const void* psi2, double d1, double d2, double* pos, void* pres, void* stream);
/* fb_cola_force: count = fb_paint(pos, weights 1, CIC); delta = count - 1; force (NULL: stop there) = c2r(coef i k delta(k) /
 *   k^2) per component, coef = (3/2) Omega_m.  No window deconvolution.                                                     */
int fb_cola_force(fb_plan* plan, const double* pos, void* count, void* delta, void* force, double coef, void* work_half1,
                  void* work_half2, void* stream);
/* fb_cola_kick: per particle, F = the CIC readout of force at pos (fb_paint's nodes and weights); per component
 *   pres += (F cK - dP1 psi1) - dP2 psi2, then (drift != 0) pos = wrap(pos + (pres Dr + dD1 psi1) + dD2 psi2).
 *   coef: HOST double[6] = {cK, dP1, dP2, Dr, dD1, dD2}.                                                                      */
int fb_cola_kick(fb_plan* plan, const void* force, const void* psi1, const void* psi2, void* pres, double* pos, const double* coef,
                 int drift, void* stream);
/* fb_cola_velocity: out[i stride] = fac ((pres + P1 psi1) + P2 psi2) of one component (0, 1, 2), DEVICE double; with
 *   fac = 100 h / a this is the peculiar velocity a dx/dt in km/s.
 * fb_cola_grid_velocity: num_inout = num_inout / count where count != 0, else 0 -- with num_inout = fb_paint(pos, v, CIC)
 *   and count = fb_paint(pos, NULL, CIC) the mass-weighted CIC velocity on the mesh.                                          */
int fb_cola_velocity(fb_plan* plan, const void* psi1, const void* psi2, const void* pres, int component, double P1, double P2,
                     double fac, double* out, int stride, void* stream);
int fb_cola_grid_velocity(fb_plan* plan, void* num_inout, const void* count, void* stream);
/* fb_cola_run: the whole run.  coef: HOST double[3 + 6 (n_steps + 1)] (fastbox_amd/cola.py launch_table) =
 *   {d1, d2, (3/2) Omega_m, then one fb_cola_kick row per launch}.  fb_cola_lpt (force as work3); fb_cola_init(d1, d2);
 *   n_steps == 0: fb_cola_force without the force (count and delta only); else n_steps + 1 times fb_cola_force then
 *   fb_cola_kick with row j, drifting in all launches but the last.  Leaves count, delta at the final positions, and pos, pres,
 *   psi1, psi2 for fb_cola_velocity.                                                                                         */
int fb_cola_run(fb_plan* plan, const void* delta0, int n_steps, const double* coef, double* pos, void* psi1, void* psi2, void* pres,
                void* force, void* count, void* delta, void* work_half1, void* work_half2, void* stream);

/* ---- void finding (fastbox/voids.py, examples/example_void_detection.py; definitions in DESIGN.md section 4) ---------------
 * One box on one GPU.  Labels are DEVICE int32[N^3] in C order; neighbours are the 6 face neighbours; the box is not periodic.
 * fb_watershed: steepest descent on the strict order (f, i), f as stored: every voxel inside the mask points to the least of
 *   itself and its in-mask face neighbours; the pointers are followed to their root (a minimum); label = 1 + the rank of the
 *   root among all minima in raster order, 0 outside the mask.  Inside: f finite and, by mask_kind, FB_VOID_MASK_ALL: always;
 *   _THRESHOLD: (double) f <= mask_threshold; _U8: mask (DEVICE uint8[N^3]) != 0; _FIELD: mask (DEVICE field of the plan's
 *   precision) != 0.  *n_regions = the number of minima.  N^3 < 2^31 (N <= 1290), since a parent word holds a voxel index
 *   in 31 bits: FB_ERR_INVALID beyond.  Synchronises (one read-back per pointer-jumping round).
 * fb_region_stats: per label l = 0..n_labels, stats_out (DEVICE, 11 columns of n_labels + 1 eight-byte words): int64 count,
 *   arg-min in (f, i) order (-1: none), sums of ix, iy, iz; double sum f, sum w, sums of w ix, w iy, w iz (w = max(-f, 0)),
 *   mean f = sum f / count.  field NULL: counts and index sums only.  A non-finite voxel of label 0 adds to its count and index
 *   sums only.  The double sums are fixed-point accumulations, the same bit for bit from call to call.  *bad |= 1 if field is
 *   not finite in a voxel of label >= 1, |= 2 if a label lies outside 0..n_labels.  Synchronises.
 * fb_merge_regions: labels_out = the connected components of the graph whose nodes are the labels >= 1 and whose edges join
 *   face-neighbouring labels i != j with |means[i] - means[j]| < threshold (means: DEVICE double[n_labels + 1]), numbered
 *   1..M in the order of their least label; 0 stays 0.  *n_merged = M.  Synchronises (one read-back per round).
 * fb_stack_voids: void v has label void_labels[v] and geom[4 v .. 4 v + 3] = centre x, y, z and radius (DEVICE).  Its point
 *   (a, b, c) is p = centre + radius (grid[b], grid[a], grid[c]) (grid: DEVICE double[grid_pix]), u = (p - axes[0, 2, 4]) /
 *   axes[1, 3, 5] per axis (axes: HOST x0, dx, y0, dy, z0, dz); it is valid if the 8 voxels floor(u) + {0, 1}^3 lie in the
 *   box and carry the void's label, and the trilinear value of field there is finite.  mean_out (DEVICE double[grid_pix^3]):
 *   the mean over the voids of the valid values (NaN: none); count_out (DEVICE int64): their number; hit_out[v] (DEVICE
 *   int32): 1 if void v has a valid point.  Sums in a fixed order.  Asynchronous.                                           */
#define FB_VOID_MASK_ALL 0
#define FB_VOID_MASK_THRESHOLD 1
#define FB_VOID_MASK_U8 2
#define FB_VOID_MASK_FIELD 3
int fb_watershed(fb_plan* plan, const void* field, int mask_kind, double mask_threshold, const void* mask, int32_t* labels_out,
                 int64_t* n_regions, void* stream);
int fb_region_stats(fb_plan* plan, const int32_t* labels, int64_t n_labels, const void* field, void* stats_out, int* bad,
                    void* stream);
int fb_merge_regions(fb_plan* plan, const int32_t* labels, int64_t n_labels, const double* means, double threshold,
                     int32_t* labels_out, int64_t* n_merged, void* stream);
int fb_stack_voids(fb_plan* plan, const int32_t* labels, const void* field, const int32_t* void_labels, const double* geom,
                   int64_t n_voids, const double* axes, const double* grid, int grid_pix, double* mean_out, int64_t* count_out,
                   int32_t* hit_out, void* stream);

/* ---- friends-of-friends halos of a particle set (nbodykit's FOF; definition in DESIGN.md section 4) --------------------------
 * One box on one GPU; particle data are fp64 whatever the plan's precision.  pos: DEVICE double[n][3] in Mpc, periodic in the
 * plan's box, wrapped on read (w = x - L floor(x / L); w < 0: w += L; w >= L: w -= L).  i != j are friends iff
 * d^2 = (dx dx + dy dy) + dz dz < link^2, d_a the minimum-image difference of the wrapped coordinates (d > L/2: d - L;
 * d < -L/2: d + L); a group is a connected component, its root its least member index.  0 <= n <= 2^31 - 2.
 * fb_fof_work_bytes: bytes of fb_fof_link's work buffer for n particles in ncells cells (-1: bad arguments).
 * fb_fof_link: root_out (DEVICE uint32[n]) = the root of every particle.  ncell: HOST int[3], cells per axis, each of side
 *   L_a / ncell_a >= link (so that friends lie in adjacent cells), at most 2^31 cells; 0 < link < min(L) / 2.  *bad = 1 (and
 *   nothing linked) if a position is not finite, has |x| >= 2^52 L (where x - L floor(x / L) is off by units of ulp(x) >= L),
 *   or does not wrap into [0, L) all the same: such a particle enters no cell.  stage_ms: HOST double[4] or NULL:
 *   milliseconds of binning, the pair search of tile 0 of every cell, the pair search of the further tiles of the cells that
 *   hold more than 64 particles, and flattening.  FB_ERR_STATE if a find / union loop (cap n + 1 steps, which a sound forest
 *   cannot reach) or the flattening hits its iteration cap.  Synchronises.
 * fb_fof_sizes: count_out (DEVICE uint32[n]) = members of the group at its root's index, 0 elsewhere; kept_out (DEVICE
 *   uint32[floor(n / nmin)][2]) = (root, count) of the groups with count >= nmin, in arbitrary order; out_host[2] = the number
 *   of groups of any size, the number kept.  work: DEVICE, 256 bytes.  Synchronises.
 * fb_fof_catalogue: the n_kept groups in the caller's order (sorted_roots, sorted_counts: DEVICE uint32[n_kept]).
 *   labels_out (DEVICE int32[n]) = the position of the particle's group in that order, -1 if it is not kept; pos_out (DEVICE
 *   double[n_kept][3]) = wrap(a + mean_i(minimum-image(w_i - a))), a the root's wrapped position; vel_out the plain mean of
 *   vel (DEVICE double[n][3]; NULL: none).  The sums are fixed-point (two 64-bit words, at least 93 - ceil(log2(n max(L) / 2))
 *   fractional bits): the same bit for bit from call to call.  *bad = 4 if a velocity, or n max |v|, is not finite.  work: DEVICE,
 *   256 + 96 n_kept bytes.  Synchronises only when vel is given.                                                              */
int64_t fb_fof_work_bytes(int64_t n, int64_t ncells);
int fb_fof_link(fb_plan* plan, const double* pos, int64_t n, double link, const int* ncell, void* work, int64_t work_bytes,
                uint32_t* root_out, int* bad, double* stage_ms, void* stream);
int fb_fof_sizes(fb_plan* plan, const uint32_t* root, int64_t n, int64_t nmin, void* work, uint32_t* count_out, uint32_t* kept_out,
                 int64_t* out_host, void* stream);
int fb_fof_catalogue(fb_plan* plan, const double* pos, const double* vel, const uint32_t* root, int64_t n,
                     const uint32_t* sorted_roots, const uint32_t* sorted_counts, int64_t n_kept, void* work, int32_t* labels_out,
                     double* pos_out, double* vel_out, int* bad, void* stream);

/* ---- pair counts in separation bins (nbodykit's SimulationBox2PCF) ------------------------------------
 * One box on one GPU; particle data are fp64 whatever the plan's precision.  pos1, pos2: DEVICE double[n][3] in Mpc, periodic
 * in the plan's box, wrapped on read and differenced by minimum image exactly as fb_fof_link does.  pos2 NULL: auto-counts
 * (ordered pairs i != j of pos1, every unordered pair twice, no particle with itself, distinct particles at one position do
 * pair; n2 is ignored); else cross-counts: all n1 n2 ordered pairs, coincident ones included.  0 <= n <= 2^31 - 2 each.
 * mode 0: bins in r -- radial bin b holds a pair iff edges2[b] <= d^2 < edges2[b + 1], d^2 = (dx dx + dy dy) + dz dz;
 *   nsub = 1.  mode 1: bins in (r, mu), mu bin m = the number of j in 1 .. nsub - 1 with dz dz (double)(nsub nsub) >=
 *   (double)(j j) d^2, every product rounded on its own (a pair with d^2 = 0 lands in m = nsub - 1).  mode 2: bins in
 *   (r_p, pi): r_p^2 = dx dx + dy dy takes the place of d^2 in the radial test, the pi bin is the number of j in
 *   1 .. nsub - 1 with dz dz >= (double)(j j), and a pair with dz dz >= sub_max^2 is dropped; sub_max = pimax = nsub.
 *   No square root is taken.  edges2: HOST double[nr + 1], the squares of the edges, strictly ascending from >= 0;
 *   1 <= nr <= 256, nr nsub <= 4096.  The largest separation along every axis (sqrt(edges2[nr]); pimax along z in mode 2)
 *   must stay below L_a / 2.  ncell: HOST int[3], cells per axis, at least 2 and of side L_a / ncell_a >= that separation.
 * fb_pair_work_bytes: bytes of fb_pair_count's work buffer (n2 = 0 for auto-counts; -1: bad arguments).
 * fb_pair_count: counts_out (DEVICE uint64[nr][nsub]) = the counts, all integer adds: the same bit for bit from call to
 *   call.  *bad = 1 (and nothing counted) if a position of either catalogue is not finite or has |x| >= 2^52 L.  stage_ms: HOST
 *   double[3] or NULL: milliseconds of binning, the sweep over tile 0 of every cell, and the sweep over the further tiles of
 *   the cells that hold more than 64 particles.  Synchronises.                                                              */
int64_t fb_pair_work_bytes(int64_t n1, int64_t n2, int64_t ncells);
int fb_pair_count(fb_plan* plan, const double* pos1, int64_t n1, const double* pos2, int64_t n2, int mode, const double* edges2,
                  int nr, int nsub, double sub_max, const int* ncell, void* work, int64_t work_bytes, uint64_t* counts_out,
                  int* bad, double* stage_ms, void* stream);

/* ---- radial profiles and aperture moments around given centres (spherical-overdensity halos) ----------
 * One box on one GPU; particle data are fp64 whatever the plan's precision.  pos, centres: DEVICE double[.][3] in Mpc, periodic
 * in the plan's box, wrapped on read; d = the minimum-image difference (particle - centre) of the wrapped coordinates exactly
 * as fb_fof_link and fb_pair_count take it, d^2 = (dx dx + dy dy) + dz dz with every operation rounded on its own.  No square
 * root is taken in any comparison.  All particles count, a particle that coincides with the centre included (d^2 = 0).
 * 0 <= n <= 2^31 - 2, 0 <= nh <= 2^31 - 2.
 * fb_profile_work_bytes: bytes of the work buffer for n particles in ncells cells (-1: bad arguments): 28 n bytes, and 28 n
 *   more with velocities, beside 8 bytes per cell.
 * fb_profile_bin: bins the particles once into ncell (HOST int[3]: at least 2 cells per axis, at most 2^31 in all) and leaves
 *   in `work` the wrapped positions in cell order, the cell table and -- vel (DEVICE double[n][3]) not NULL -- the velocities
 *   in the same order (a permuted copy), for any number of the two sweeps below.  *bad = 1 if a position is not finite or has
 *   |x| >= 2^52 L; *bad = 4 if a velocity, or 3 n max|v|^2, is not finite; the buffer is then not prepared.  stage_ms: HOST
 *   double[1] or NULL: milliseconds of the binning.  Synchronises.
 * fb_halo_profiles: counts_out (DEVICE uint32[nh][nr + 1]): column 0 of row h = #{i : d^2 < edges2[0]}, column b + 1 =
 *   #{i : edges2[b] <= d^2 < edges2[b + 1]}.  edges2: HOST double[nr + 1], the squares of the edges, strictly ascending from
 *   >= 0; 1 <= nr <= 256.  The reach sqrt(edges2[nr]) must stay below L_a / 2 and within the side L_a / ncell_a of the cells
 *   binned (the caller leaves the margin for the rounding of a cell index: pair_cells of halos.py).  Integer counts: the same
 *   bit for bit from call to call and for any order of the particles.  *bad = 1 if a centre is not finite or has
 *   |x| >= 2^52 L (the rows are then undefined).  Synchronises.
 * fb_halo_apertures: per centre h the particles with d^2 < r2[h] (r2: DEVICE double[nh]): count_out (DEVICE uint32[nh]) = their
 *   number m; com_out (DEVICE double[nh][3]) = wrap(c + sum d / m), c the wrapped centre; with vmean_out (DEVICE
 *   double[nh][3]) and sigma_out (DEVICE double[nh]) -- both or neither, and only on a buffer binned with velocities --
 *   vmean = sum v / m and sigma = sqrt(max(0, (sum v.v / m - vmean.vmean) / 3)), v.v = (vx vx + vy vy) + vz vz; m = 0: NaN.
 *   The sums are fixed-point in two 64-bit words with F = 93 - e fractional bits, bound < 2^e (frexp), the bound being
 *   n max(L) / 2 for the offsets, n max|v| for the velocities and 3 n max|v|^2 for v.v: the same bit for bit from call to
 *   call and for any order of the particles.  reach >= every sqrt(r2[h]), under the same limits as the reach of the profiles;
 *   *bad has bit 8 set if some r2[h] > reach^2 (or is NaN) and bit 1 for a bad centre; the outputs of such a centre are not
 *   written.  Synchronises.                                                                                                  */
int64_t fb_profile_work_bytes(int64_t n, int64_t ncells, int with_vel);
int fb_profile_bin(fb_plan* plan, const double* pos, int64_t n, const double* vel, const int* ncell, void* work, int64_t work_bytes,
                   int* bad, double* stage_ms, void* stream);
int fb_halo_profiles(fb_plan* plan, void* work, const double* centres, int64_t nh, const double* edges2, int nr,
                     uint32_t* counts_out, int* bad, void* stream);
int fb_halo_apertures(fb_plan* plan, void* work, const double* centres, const double* r2, int64_t nh, double reach,
                      uint32_t* count_out, double* com_out, double* vmean_out, double* sigma_out, int* bad, void* stream);

/* ---- three-point correlation multipoles of a catalogue (nbodykit's SimulationBox3PCF) -----------------
 * One box on one GPU; particle data are fp64 whatever the plan's precision.  pos: DEVICE double[n][3] in Mpc, periodic in the
 * plan's box, wrapped on read; w: DEVICE double[n], weights of any sign, or NULL: all 1.  d = the minimum-image difference
 * x_j - x_i of the wrapped coordinates exactly as fb_fof_link and fb_pair_count take it, d^2 = (dx dx + dy dy) + dz dz with every
 * operation rounded on its own.  Particle j != i -- by index, not by position -- is in bin b of primary i iff edges2[b] <= d^2 <
 * edges2[b + 1]; edges2: HOST double[nr + 1], the squares of the edges, strictly ascending from > 0, so that a particle with
 * d^2 < edges2[0], a coincident one included, is in no bin and no direction of a zero vector is formed.  The unit vector is
 * (x, y, z) = d / sqrt(d^2), component by component.  Real orthonormal harmonics by this recurrence (+ - x / sqrt only):
 *   c_0 = 1, s_0 = 0, c_m = x c_(m-1) - y s_(m-1), s_m = x s_(m-1) + y c_(m-1);
 *   A_0 = sqrt(1 / (4 pi)), A_m = A_(m-1) sqrt((2 m + 1) / (2 m)); Q_m^m = A_m; Q_(m+1)^m = (sqrt(2 m + 3) z) Q_m^m;
 *   Q_l^m = alpha_lm (z Q_(l-1)^m - beta_lm Q_(l-2)^m), alpha_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),
 *   beta_lm = sqrt(((l - 1)^2 - m^2) / (4 (l - 1)^2 - 1));
 *   Y_l0 = Q_l^0, Y_l,+m = (sqrt(2) Q_l^m) c_m, Y_l,-m = (sqrt(2) Q_l^m) s_m; index lm = l^2 + l + m.
 * The constants are formed once on the host in fp64.  Per primary i and bin b: a_lm(b) = sum_j w_j Y_lm, N(b) = #{j in b},
 * S(b) = sum_j w_j^2, and
 *   M_l(b1, b2) = sum_i w_i ((4 pi / (2 l + 1)) sum_m a_lm(b1) a_lm(b2) - [b1 = b2] S(b1)),
 * the sum over m in ascending order in fp64 -- by the addition theorem the sum over ordered triplets (i; j != k) of
 * w_i w_j w_k P_l(u_ij . u_ik).  Every sum over particles is fixed-point in two 64-bit words with F = 93 - e fractional bits,
 * bound < 2^e (frexp), the bound being 2 n wmax for the a_lm, n wmax^2 for S and 4 (n wmax)^3 for M, wmax = max |w| (1 without
 * weights): the same bit for bit from call to call and for any order of the particles.
 * Limits: 0 <= n <= 2^31 - 2, 1 <= nr <= 32, 0 <= lmax <= 10 (lmax = 10 with nr = 32 takes 149 KiB of the CU's LDS).  ncell:
 * HOST int[3], cells per axis, at least 2 and of side L_a / ncell_a >= sqrt(edges2[nr]), which must stay below L_a / 2 (the
 * caller leaves the margin for the rounding of a cell index: pair_cells of halos.py).
 * fb_triplet_work_bytes: bytes of the work buffer (-1: bad arguments): 32 n bytes, 8 n more with weights, 8 bytes per cell and
 *   8 KiB x (lmax + 1) nr (nr + 1) / 2 for the workgroups' partial sums.
 * fb_triplet_multipoles: M_out (DEVICE double[lmax + 1][nr][nr], symmetric in the bins); pairs_out (DEVICE uint64[nr]) =
 *   sum_i N_i(b), the ordered pairs of fb_pair_count's auto-counts.  probe_idx: HOST int32[nprobe], nprobe <= 64 (0: none): the
 *   a_lm of these primaries, given by their index in pos, go to alm_out (DEVICE double[nprobe][(lmax + 1)^2][nr]).  *bad = 1
 *   (and all outputs zero) if a position is not finite or has |x| >= 2^52 L; *bad = 4 if a weight, or 4 (n wmax)^3, is not
 *   finite.  stage_ms: HOST double[3] or NULL: milliseconds of the binning, the sweep and the finish.  Synchronises.         */
int64_t fb_triplet_work_bytes(int64_t n, int64_t ncells, int nr, int lmax, int weighted);
int fb_triplet_multipoles(fb_plan* plan, const double* pos, const double* w, int64_t n, const int* ncell, const double* edges2,
                          int nr, int lmax, void* work, int64_t work_bytes, double* M_out, uint64_t* pairs_out,
                          const int32_t* probe_idx, int nprobe, double* alm_out, int* bad, double* stage_ms, void* stream);

/* ---- transfer functions (apply_transfer_fn box.py:374-379, smooth_field :651-653) ---------- */
#define FB_FILT_TABLE 0          /* table: real multiplier, same layout as the field */
#define FB_FILT_BEAM_HIGHPASS 1  /* (1-exp(-.5(|kpar|/p0)^p2)) [p0>0] * exp(-.5(kperp/p1)^2) [p1>0] */
#define FB_FILT_WEDGE 2          /* 0 where |kpar| < p0*kperp + p1, else 1 */
#define FB_FILT_TOPHAT 3         /* 3(sin x - x cos x)/x^3, x = |k| p0 */
/* out = nan_to_num(in * T(kperp, kpar)); layout 0 = full, 1 = half; in == out allowed */
int fb_apply_filter(fb_plan* plan, const void* in, void* out, int layout, int kind, const double* params,
                    const void* table_dev, void* stream);

/* ---- velocity / potential (box.py:251-284, 347-348) ------------------------------------------ */
int fb_velocity_k(fb_plan* plan, const void* dk, void* out, int layout, int component, double fac, void* stream);
int fb_potential_k(fb_plan* plan, const void* dk, void* out, int layout, void* stream);

/* ---- real-space operators ---------------------------------------------------------------------- */
/* out = exp(in)/mean(exp(in)) - 1 (box.py:457-460), formed as exp(in - max in)/mean(exp(in - max in)) - 1 so that
 * no intermediate leaves the plan's floating-point range; *mean_out receives mean(exp(in)). Synchronises. */
int fb_lognormal(fb_plan* plan, const void* real_in, void* real_out, double* mean_out, void* stream);
/* largest finite value of a real field (the exact shift of a fused log-normal transform, fb_set_exp_shift).
 * Synchronises. */
int fb_max_real(fb_plan* plan, const void* real, double* out, void* stream);
/* redshift_space_density (box.py:405-437). noise: T[N][N][N] standard normals in LOS order
 * (parity) or NULL -> Philox stream 1 of `seed` when sigma_nl > 0.  method: what box.py:433-437 hands to
 * scipy's griddata -- 'linear' (the default; points outside the shifted samples get the end-point average),
 * 'nearest' (no fill: scipy extrapolates with the end samples) or 'cubic' (the not-a-knot cubic spline through the
 * sorted shifted samples, the end-point average outside them; a line with two EQUAL shifted coordinates -- scipy raises
 * there -- comes back non-finite).                                                                          */
#define FB_RSD_LINEAR 0
#define FB_RSD_NEAREST 1
#define FB_RSD_CUBIC 2        /* griddata(method='cubic') in 1-D: the not-a-knot cubic spline through the sorted shifted samples */
int fb_redshift_space(fb_plan* plan, const void* delta, const void* vz, const void* noise, void* out,
                      double Hz, double sigma_nl, uint64_t seed, int method, void* stream);
/* sum(x) / sum(x^2) over a real field; sum |dk|^2 over the FULL grid from a half spectrum
 * (test_parseval, box.py:944-946).  Synchronise.                                                    */
int fb_sum_real(fb_plan* plan, const void* real, int squared, double* out, void* stream);
int fb_sumsq_half(fb_plan* plan, const void* half, double* out, void* stream);

/* ---- layout conversion -------------------------------------------------------------------------- */
int fb_expand_half(fb_plan* plan, const void* half, void* full, void* stream);  /* Hermitian extension */
int fb_crop_full(fb_plan* plan, const void* full, void* half, void* stream);    /* keep k_z <= N/2      */

/* ---- per-kernel timing with HIP events on the launch stream ---------------------------------------- */
#define FB_PROF_FFT_STRIDED 0   /* x / y passes of the 3-D FFT            */
#define FB_PROF_FFT_CONTIG 1    /* z pass (c2c, r2c, c2r)                 */
#define FB_PROF_COLOUR 2
#define FB_PROF_BIN 3
#define FB_PROF_FILTER 4
#define FB_PROF_VELPOT 5
#define FB_PROF_REALOP 6
#define FB_PROF_RSD 7
#define FB_PROF_LAYOUT 8
#define FB_PROF_FFT_GEN 9       /* x pass with the fused Gaussian generator */
#define FB_PROF_FFT_BIN 10      /* x pass with the fused shell binning      */
#define FB_PROF_PCA 11          /* channel covariance and projection of the PCA cleaning */
#define FB_PROF_NCAT 12
/* between start and stop every kernel launch of this plan is bracketed by an event pair;
 * stop synchronises and returns summed milliseconds and launch counts per class above.  */
int fb_profile_select(fb_plan* plan, unsigned mask);   /* bit i = bracket class i; default all */
/* bracket only every stride-th selected launch (an event pair costs ~3 us of stream time; 1 = all, the default);
 * stride = 0 leaves the stride as it is; *seen (may be NULL) receives the number of selected launches since the last
 * fb_profile_start */
int fb_profile_sample(fb_plan* plan, int stride, int64_t* seen);
int fb_profile_start(fb_plan* plan);
int fb_profile_stop(fb_plan* plan, void* stream, double* ms, int64_t* launches, int ncat);

/* element-wise arithmetic on real cubes T[N][N][N], the callers' own numpy expressions between the steps
 * (examples/example_endtoend.py:47, :75, :86): out = a x + b y + c (y may be NULL); out = x * y.  out may alias. */
int fb_real_axpby(fb_plan* plan, const void* x, const void* y, void* out, double a, double b, double c, void* stream);
int fb_real_multiply(fb_plan* plan, const void* x, const void* y, void* out, void* stream);

/* ---- per-channel 2-D operations on a complex cube complex<T>[N][N][N] (frequency = last axis), as
 * filters.angular_bandpass_filter (fastbox/filters.py:58-90) needs them ----
 * fb_fft_transverse: np.fft.fftn(cube, axes=[0,1]) (direction -1) / np.fft.ifftn(cube, axes=[0,1]) (+1), in place.
 * fb_mask_transverse: cube[kx, ky, :] *= mask2d[kx][ky] (T[N][N] on the device; :89).                             */
int fb_real_to_complex(fb_plan* plan, const void* real_cube, void* full_cube, void* stream);
int fb_fft_transverse(fb_plan* plan, void* full_cube, int direction, void* stream);
int fb_mask_transverse(fb_plan* plan, void* full_cube, const void* mask2d, void* stream);

/* ---- beam convolution, channel by channel (BeamModel.convolve_fft / convolve_real, fastbox/beams.py:63-137) ----
 * out[n][n][n] = (field (*) beam)[mode='same'] / sum_xy beam, for real cubes field, beam of T[n][n][n] (frequency =
 * last axis).  `plan` is the plan of the TRANSFORM size M = plan N: periodic = 0: M = 2 n, zero-padded linear
 * convolution = scipy.signal.fftconvolve(beam, field, mode='same', axes=[0, 1]) (:85-87); periodic = 1: M = n,
 * circular convolution = scipy.signal.convolve2d(beam[:, :, i], field[:, :, i], mode='same', boundary='wrap')
 * (:134-136).  work_a, work_b: distinct device buffers of complex<T>[M][M][n].  work_b holds the beam's transform
 * afterwards: beam_ready = 1 on a later call with the same plan, mode and work_b reuses it (beam is then ignored). */
int fb_beam_convolve(fb_plan* plan, const void* field, const void* beam, void* work_a, void* work_b, void* out,
                     int periodic, int beam_ready, void* stream);

/* ---- PCA foreground cleaning of a data cube T[N][N][N] (frequency = last axis), fastbox/filters.py:93-183 ----
 * mean_dev[N]: per-channel mean over the N^2 pixels (:142), fp64 on the DEVICE.                                   */
int fb_channel_means(fb_plan* plan, const void* cube, double* mean_dev, void* stream);
/* cov_dev[N][N] = np.cov of the mean-subtracted channels (:157-158; divisor N^2 - 1), fp64 on the DEVICE, formed on
 * the fp64 matrix cores (v_mfma_f64_16x16x4_f64) with a fixed summation order.  Its leading eigenvectors
 * (:161-169; an N x N problem): fb_leading_eigenvectors below, or the caller's own solver -- modes_dev[N][nmodes].   */
int fb_channel_covariance(fb_plan* plan, const void* cube, const double* mean_dev, double* cov_dev, void* stream);
/* The split of the N^2 pixels that fb_channel_covariance uses on a device of num_cu compute units, on the host and without a
 * device: slice q of *slices_out covers the pixels [q rows, min((q + 1) rows, N^2)) with rows = *rows_out a multiple of 4; every
 * slice is non-empty and they tile [0, N^2).  The partial sums of the slices are added in slice order.  FB_ERR_INVALID for
 * N < 2, num_cu < 1 or a null output.                                                                                      */
int fb_channel_covariance_plan(int N, int num_cu, int* slices_out, int64_t* rows_out);
/* The nmodes leading eigenpairs of cov_dev[N][N] (symmetric, fp64, DEVICE; not modified) -- np.linalg.eig + the sort by
 * decreasing eigenvalue of :161-169 -- by cyclic two-sided Jacobi in fp64 on the device (round-robin ordering, N/2
 * rotations per launch; 6-10 sweeps): modes_dev[N][nmodes] (orthonormal columns, the sign of a column is not defined,
 * as with LAPACK), vals_dev[nmodes] (descending; may be NULL), *sweeps_out (host; may be NULL).  Equal eigenvalues keep
 * the order of their diagonal positions.  Synchronises the stream (one convergence check per sweep).  FB_ERR_INVALID
 * for a matrix with non-finite entries, FB_ERR_STATE if 60 sweeps do not converge.  0 <= nmodes <= N.                 */
int fb_leading_eigenvectors(fb_plan* plan, const double* cov_dev, int nmodes, double* modes_dev, double* vals_dev,
                            int* sweeps_out, void* stream);
/* cube_out = cube - (U (U^T x) + mean), x = cube - mean (:172-176); amps_dev[nmodes][N^2] = U^T x (:172) or NULL   */
int fb_pca_clean(fb_plan* plan, const void* cube, const double* mean_dev, const double* modes_dev, int nmodes,
                 void* cube_out, double* amps_dev, void* stream);

/* ---- NMF and ICA foreground cleaning (fastbox/filters.py:373-432, :187-243) ----
 * The cube is T[N][N][N] in the plan's precision, frequency last; all other state is fp64.  W_dev[k][N^2] and X1_dev[n][N^2]
 * have the layout of fb_pca_clean's amps_dev; H_dev[k][N] holds one component's spectrum contiguously.  1 <= k, n <= 16
 * (FB_ERR_INVALID otherwise).  Every sum is taken in a fixed order without atomics: results are bitwise repeatable.
 *
 * fb_real_min: *min_out = the least value of a real cube (NaN is skipped), *nonfinite_out = the number of NaN / infinite
 *   values: the admissibility test of NMF without a download.  Synchronises.
 * fb_complex_to_real: real_cube = Re full_cube (complex<T>[N][N][N] -> T[N][N][N]).                                       */
int fb_real_min(fb_plan* plan, const void* cube, double* min_out, int64_t* nonfinite_out, void* stream);
int fb_complex_to_real(fb_plan* plan, const void* full_cube, void* real_cube, void* stream);
/* fb_nmf_sweep: ONE iteration of scikit-learn's coordinate-descent solver (Frobenius loss, no regularisation, no shuffling)
 *   for X ~ W H, X[N^2][N] = the cube: with H H^T and X H^T every row of W is swept cyclically,
 *     grad = -(X H^T)[i][t] + sum_r (H H^T)[t][r] W[i][r];  violation += |grad|, or |min(0, grad)| where W[i][t] == 0;
 *     W[i][t] = max(W[i][t] - grad / (H H^T)[t][t], 0) unless that diagonal entry is 0,
 *   then the rows of H^T likewise with W^T W and X^T W of the new W.  The cube is read once: the pass that sweeps a pixel's
 *   row of W also adds the pixel to X^T W and W^T W.  W_dev and H_dev are updated in place; violation_out[2] (host) = the
 *   violations of the W half and of the H half.  N <= 1024 (FB_ERR_UNSUPPORTED beyond).  Synchronises.
 * fb_nmf_residual: cube_out = X - W H (may be NULL), *sumsq_out (host; may be NULL) = ||X - W H||_F^2 in fp64; synchronises
 *   if sumsq_out is given.
 * fb_nndsvd_norms: out[2 j], out[2 j + 1] (host) = the sums of squares of the positive and of the negative entries of
 *   row j of amps_dev[k][N^2] (the NNDSVD rule needs the norms of both parts of every singular vector).  Synchronises.
 * fb_nndsvd_fill: amps_dev[j][p] <- max(coef[j] amps_dev[j][p], 0) (row 0: the absolute value if abs_first), then every value
 *   below eps becomes `fill` (NNDSVDA: the mean of X).  coef[k] on the host.
 * fb_rotated_covariance: cov_dev[N][N] = B^T B / (N^2 - 1) for B[p][m] = sum_c Vt_dev[m][c] X[p][c], the spectra in the basis
 *   of the N rows of Vt_dev[N][N] (fp64), formed and kept in fp64 for both plans and not centred.  With Vt the eigenvectors of
 *   X^T X, B has nearly orthogonal columns, so that the singular values and vectors of X follow from this matrix without the
 *   loss of the Gram matrix.  work_dev: N^3 + N doubles.                                              */
int fb_nmf_sweep(fb_plan* plan, const void* cube, double* W_dev, double* H_dev, int k, double* violation_out, void* stream);
/* The pixel partitions of fb_nmf_sweep (on a device of num_cu compute units) and of fb_ica_step, on the host and without a device:
 * workgroup q of *workgroups_out takes the pixels [q per, min((q + 1) per, N^2)), per = *pixels_out; a workgroup whose share starts
 * at or past N^2 is empty and contributes zeros.  The workgroups' partial sums are added in workgroup order.  The sweep's `per` is
 * a multiple of 4.  FB_ERR_INVALID for N < 2 (the sweep: N > 1024), num_cu < 1 or a null output.                              */
int fb_nmf_sweep_plan(int N, int num_cu, int* workgroups_out, int64_t* pixels_out);
int fb_ica_step_plan(int N, int* workgroups_out, int64_t* pixels_out);
int fb_nmf_residual(fb_plan* plan, const void* cube, const double* W_dev, const double* H_dev, int k, void* cube_out,
                    double* sumsq_out, void* stream);
int fb_nndsvd_norms(fb_plan* plan, const double* amps_dev, int k, double* out, void* stream);
int fb_nndsvd_fill(fb_plan* plan, double* amps_dev, int k, const double* coef, int abs_first, double eps, double fill,
                   void* stream);
int fb_rotated_covariance(fb_plan* plan, const void* cube, const double* Vt_dev, double* work_dev, double* cov_dev, void* stream);
/* fb_ica_step: the sums of one FastICA fixed-point step (algorithm 'parallel') for the unmixing matrix W[n][n] (host) and
 *   the whitened data X1_dev: G_out[n][n] = g(W X1) X1^T / N^2 and gp_out[n] = mean over pixels of g'((W X1)_i) (host), with
 *   g = tanh(alpha y) (FB_ICA_LOGCOSH), y exp(-y^2 / 2) (FB_ICA_EXP) or y^3 (FB_ICA_CUBE).  Synchronises.
 * fb_ica_sources: sources_dev[i][p] = scale[i] (W X1)[i][p]; moments_out[2 n] (host; may be NULL) = the mean over pixels of
 *   every row of sources_dev, then the mean of its square.  W[n][n], scale[n] on the host.  Synchronises.                  */
#define FB_ICA_LOGCOSH 0
#define FB_ICA_EXP 1
#define FB_ICA_CUBE 2
int fb_ica_step(fb_plan* plan, const double* W, const double* X1_dev, int n, int fun, double alpha, double* G_out,
                double* gp_out, void* stream);
int fb_ica_sources(fb_plan* plan, const double* W, const double* scale, const double* X1_dev, int n, double* sources_dev,
                   double* moments_out, void* stream);

/* ---- in-painting of flagged channels by Gaussian constrained realisations (fastbox/inpaint.py:35-155), fb_inpaint.hip ----
 * For every line of sight p (a row of the (N^2, N) view of the cube) with flags w, diagonal noise variance sigma^2, signal
 * prior S and q = w^2 / sigma^2:  A_p x_p = b_p,  A_p = I + S^(1/2) diag(q_p) S^(1/2),
 * b_p = S^(1/2) (q_p d_p + sqrt(q_p) omega2) + omega1,  s_p = S^(1/2) x_p  (DESIGN.md section 4).  Cubes called fp64 below are
 * double[N^2][N] on the DEVICE whatever the plan's precision; N <= 1024.
 *
 * fb_los_matmul: Y[p][a] = post[p][a] sum_b M_dev[a][b] (pre[p][b] X[p][b]) + add[p][a] on the fp64 matrix cores
 *   (v_mfma_f64_16x16x4_f64).  M_dev[N][N] fp64, not assumed symmetric.  X: a cube in the plan's precision (FB_LOS_X_PLAN) or
 *   fp64 (FB_LOS_X_FP64); pre, post, add: fp64 cubes or NULL; Y: fp64 cube, distinct from X and pre (add == Y is allowed).
 * fb_gcr_rhs: q_out = w^2 / var (exactly 0 where w = 0), u_out = q d + sqrt(q) omega2 (0 where w = 0: d is selected, not
 *   multiplied, so a NaN under a flag is legal).  d: cube in the plan's precision.  w: such a cube (FB_GCR_PER_VOXEL) or
 *   double[N] on the device (FB_GCR_PER_CHANNEL); var: double[N] on the device (FB_GCR_PER_CHANNEL) or a cube in the plan's
 *   precision (FB_GCR_PER_VOXEL).  draws: FB_GCR_DRAWS_NONE (omega = 0: the Wiener filter), FB_GCR_DRAWS_GIVEN (omega2: fp64
 *   cube of unit normals; omega1 stays with the caller) or FB_GCR_DRAWS_DEVICE (element p N + c of Philox streams 7 (omega1,
 *   written to omega1_out) and 8 (omega2) under (seed, realisation)).  qmean_dev[N] (device; may be NULL): the mean of q over
 *   the pixels of every channel, summed as fb_channel_means does.
 * fb_gcr_solve: batched preconditioned conjugate gradients from x = 0 over all N^2 rows for A x = b with the preconditioner
 *   P_dev[N][N] (symmetric positive definite; NULL: none).  A row stops once its recurrence residual |r| <= tol |b| and is
 *   then left alone; a row with b = 0 takes no iteration.  The loop ends when no row is active or after maxiter iterations;
 *   one count is read back per iteration.  work: 5 N^3 doubles (4 N^3 without P_dev).  n_iter_dev[N^2]: iterations per row.
 *   info_out[4] (host): max_p |b - A x| / |b| from one more application of A, the number of rows that met the tolerance,
 *   the largest iteration count of a row, the iterations of the loop.  Synchronises.
 * fb_gcr_finish: cube_out = S^(1/2) x (s_work: fp64 scratch cube, not x) + sqrt(var) omega3 (noise: FB_GCR_DRAWS_NONE, _GIVEN
 *   with omega3 an fp64 cube, or _DEVICE: Philox stream 9), stored in the plan's precision; with `inpaint`, d where w != 0
 *   (bit for bit) and that value elsewhere.
 * fb_replace_nan_channel_mean: cube_out = cube with every NaN replaced by the mean of its channel over the voxels that are
 *   not NaN (fp64 sums in a fixed order; a channel without such a voxel stays NaN; other voxels are copied bit for bit).
 *   mean_dev[N] (device; may be NULL) receives the means.  cube_out == cube is allowed.                                      */
#define FB_LOS_X_PLAN 0
#define FB_LOS_X_FP64 1
#define FB_GCR_PER_CHANNEL 0
#define FB_GCR_PER_VOXEL 1
#define FB_GCR_DRAWS_NONE 0
#define FB_GCR_DRAWS_GIVEN 1
#define FB_GCR_DRAWS_DEVICE 2
int fb_los_matmul(fb_plan* plan, const double* M_dev, const void* X, int x_kind, const double* pre, const double* post,
                  const double* add, double* Y, void* stream);
int fb_gcr_rhs(fb_plan* plan, const void* d, const void* w, int w_kind, const void* var, int var_kind, const double* omega2,
               int draws, uint64_t seed, uint64_t realisation, double* q_out, double* u_out, double* omega1_out, double* qmean_dev,
               void* stream);
int fb_gcr_solve(fb_plan* plan, const double* sqrtS_dev, const double* P_dev, const double* q, const double* b, double* x,
                 double* work, double tol, int maxiter, int32_t* n_iter_dev, double* info_out, void* stream);
int fb_gcr_finish(fb_plan* plan, const double* sqrtS_dev, const double* x, double* s_work, const void* var, int var_kind,
                  const double* omega3, int noise, uint64_t seed, uint64_t realisation, const void* d, const void* w, int w_kind,
                  int inpaint, void* cube_out, void* stream);
int fb_replace_nan_channel_mean(fb_plan* plan, const void* cube, void* cube_out, double* mean_dev, void* stream);

/* ---- least-squares spectral analysis of flagged cubes (fastbox/inpaint.py:158-399), fb_lssa.hip ----
 * Per line of sight p and mode n, with the phase tables of the host (mode-major double[ntau][N] on the device: cos phi and
 * sin phi; the device never derives a phase) and g = taper^2 w^2 / var (exactly 0 where w = 0):
 *   A_re = sum_j g d cos / G_p,  A_im = -sum_j g d sin / G_p,  G_p = sum_j g   (d is selected away where g = 0: NaN is legal)
 *   S_cc = sum_j w^2 cos^2,  S_cs = sum_j w^2 cos sin,  S_ss = sum_j w^2 - S_cc
 *   theta = atan2(2 S_cs, S_cc - S_ss) / 2,  (A_1, A_2) = R(theta) (A_re, A_im),  l_0, l_1 = diag(R S R^T)
 *   ps = ((A_1 l_1)^2 + (A_2 l_0)^2) / (l_0^2 + l_1^2);  without `decorrelate` ps = A_re^2 + A_im^2
 * in one fused kernel on the fp64 matrix cores.  A row with G_p = 0 has A = 0 and ps = NaN and is left
 * out of the averages.  All sums in a fixed order; results are bitwise repeatable.  N <= 1024, 1 <= ntau <= 1024.
 *
 * fb_lssa: d: cube in the plan's precision.  w: such a cube (FB_GCR_PER_VOXEL) or double[N] on the device
 *   (FB_GCR_PER_CHANNEL); var: NULL (1), double[N] on the device (FB_GCR_PER_CHANNEL) or a cube in the plan's precision
 *   (FB_GCR_PER_VOXEL); taper_dev: double[N] on the device or NULL (1).  With per-channel flags the overlap sums do not
 *   depend on p and come from the host as s_dev = double[3][ntau] on the device (S_cc, S_cs, S_ss; needed with
 *   `decorrelate`, not read with per-voxel flags).  A_re, A_im, ps: double[N^2][ntau] on the device, each may be NULL
 *   (not stored).  With amps_given, A_re and A_im are inputs (d is not read, nor the tables with per-channel flags) and only ps and the
 *   averages are formed.  ps_mean_out[ntau], ps_stderr_out[ntau], n_los_out (host, each may be NULL): over the n_los rows
 *   with G_p > 0 the mean of ps and its population standard deviation / sqrt(n_los).  Synchronises.                           */
int fb_lssa(fb_plan* plan, const void* d, const void* w, int w_kind, const void* var, int var_kind, const double* taper_dev,
            const double* cos_dev, const double* sin_dev, const double* s_dev, int ntau, int decorrelate, int amps_given, double* A_re, double* A_im, double* ps, double* ps_mean_out,
            double* ps_stderr_out, long long* n_los_out, void* stream);

/* ---- model fits along the line of sight (fastbox/filters.py:494-593 gpr_filter, :598-664 LSQfitting), fb_losfit.hip ----
 * One wave per line of sight p (a row of the (N^2, N) view), all fit state fp64, every sum in a fixed order; N <= 1024.  w and
 * sigma: NULL (1 everywhere), double[N] on the device (FB_GCR_PER_CHANNEL) or a cube in the plan's precision
 * (FB_GCR_PER_VOXEL); w = 0 flags a voxel, whose datum is selected away and may be NaN.  status_dev[N^2]: FB_LOSFIT_* per row;
 * a row with a status other than FB_LOSFIT_OK is NaN in every output.  n_failed_out (host): the number of such rows.  Both fit
 * entries synchronise.  Definitions: DESIGN.md section 4.
 *
 * fb_los_polyfit: per row minimise sum_c w^2 (y_c - sum_k a_k basis_dev[k][c])^2, k = 0 .. order (order <= 7), y = T or, with
 *   log_y, ln T.  basis_dev[order + 1][N] fp64: the basis at the channels (the caller's Legendre polynomials).  pinv_dev
 *   (NULL, or [order + 1][N] fp64 with no or per-channel w): a_k = sum_c pinv_dev[k][c] y_c over the unflagged channels, the
 *   shared pseudo-inverse with w folded in; without it every row accumulates its own normal matrix and solves it by Cholesky.
 *   cube_out = T - model where w != 0 and exactly 0 elsewhere (model = exp(fit) with log_y).  model_out (may be NULL): the
 *   model at every channel, flagged ones included, in the plan's precision.  coeffs_dev (may be NULL): double[order + 1][N^2].
 *   chi2_dev (may be NULL): double[N^2], sum_c w^2 (y - fit)^2.  FB_LOSFIT_TOO_FEW: fewer unflagged channels than coefficients;
 *   _NONFINITE: a non-finite unflagged datum; _NONPOSITIVE: an unflagged datum <= 0 with log_y; _SINGULAR: a pivot <= 0.
 * fb_los_powerlaw: d = maps - tpsmean_dev[c] (NULL: 0), x = nu / nu_0 given as lnx_dev[N] = ln x.  Stage 1 minimises
 *   sum_c (w (ampS x^betaS - d) / sigma)^2 over 0.5 d0 <= ampS <= 1.5 d0 and betaS between 0.9 b and 1.1 b, d0 the first
 *   unflagged datum, b = beta_guess_dev[p] or, where that is NULL, ln(d3 / d0) / ln(x3 / x0) from the first and fourth
 *   unflagged channels: for every betaS the best ampS in its interval is closed-form, and betaS takes Gauss-Newton steps
 *   clipped to its interval and halved while the cost rises, until a step is below tol max(1, |betaS|) (at most max_iter
 *   steps, at most max_iter halvings each).  Stage 2: amps = (S^T S)^-1 S^T d on the unflagged channels, S = [x^betaS,
 *   x^freeind]; model = S amps; resid_out = d - model where w != 0 and exactly 0 elsewhere.  rows_dev: double[5][N^2] = betaS,
 *   ampS, the two amps, the stage-1 cost (half the sum of squares).  n_iter_dev[N^2]: steps taken.  FB_LOSFIT_TOO_FEW: fewer
 *   than four unflagged channels; _NONFINITE; _NONPOSITIVE: d0 <= 0 or d3 / d0 <= 0; _SINGULAR: a normal matrix is singular
 *   (stage 2: det <= 1e-14 S11 S22); _MAXITER.
 * fb_los_subtract: cube_out = X - shift_dev[c] - Y, X and cube_out cubes in the plan's precision, Y an fp64 cube: with
 *   Y = M X from fb_los_matmul and shift = mean - M mean that is (I - M)(X - mean), the cleaned cube of the Gaussian-process
 *   filter.  cube_out must not be X.                                                                                            */
#define FB_LOSFIT_OK 0
#define FB_LOSFIT_TOO_FEW 1
#define FB_LOSFIT_NONFINITE 2
#define FB_LOSFIT_NONPOSITIVE 3
#define FB_LOSFIT_SINGULAR 4
#define FB_LOSFIT_MAXITER 5
int fb_los_polyfit(fb_plan* plan, const void* cube, const void* w, int w_kind, const double* basis_dev, const double* pinv_dev,
                   int order, int log_y, void* cube_out, void* model_out, double* coeffs_dev, double* chi2_dev, int32_t* status_dev,
                   int32_t* n_failed_out, void* stream);
int fb_los_powerlaw(fb_plan* plan, const void* maps, const double* tpsmean_dev, const void* sigma, int sigma_kind, const void* w,
                    int w_kind, const double* lnx_dev, double freeind, const double* beta_guess_dev, int max_iter, double tol,
                    void* resid_out, void* model_out, double* rows_dev, int32_t* n_iter_dev, int32_t* status_dev,
                    int32_t* n_failed_out, void* stream);
int fb_los_subtract(fb_plan* plan, const void* X, const double* Y, const double* shift_dev, void* cube_out, void* stream);

/* ---- putting data onto a grid (fastbox/analysis.py:31-70 interpolate_onto_grid, :73-118 grid_catalogue), fb_regrid.hip ----
 * fb_regrid_trilinear: cube T[nx][ny][nz] (plan precision, every axis >= 2) given at the nodes gx[nx], gy[ny], gz[nz], each
 *   strictly ascending (the caller's check; any table is memory-safe), interpolated at the points px[npx], py[npy], pz[npz]
 *   (any order, each >= 1 long): scipy's RegularGridInterpolator(method='linear', bounds_error=False, fill_value=nan) behind
 *   replace_nan_with_channel_mean.  All six tables are DEVICE double; all coordinate and weight arithmetic is fp64.  Per axis:
 *     i = clip(searchsorted(g, p, 'right') - 1, 0, n - 2),  t = (p - g[i]) / (g[i + 1] - g[i]),
 *     p is inside iff g[0] <= p <= g[n - 1] (both ends closed; NaN is outside);
 *   value = sum over the eight corners, x outermost and z innermost, of v ((w_x w_y) w_z) with w = 1 - t at node i and t at
 *   node i + 1, starting from 0; zero weights are not skipped, so a NaN corner of weight 0 gives NaN.  A point outside on any
 *   axis gives NaN.  A NaN voxel of the cube reads as the mean of its channel (last axis) over the nx ny voxels that are not NaN,
 *   summed in fp64 in a fixed order (bitwise repeatable); no filled copy is written; a channel that is NaN throughout stays NaN.
 *   out: T[npx][npy][npz] or, with swap_xy, T[npy][npx][npz] -- element [j][i][k] at (px[i], py[j], pz[k]), the order of
 *   numpy's default 'xy' meshgrid that the reference returns.  Indexing is 64-bit.  Work memory: the plan's shared work buffer
 *   (npx + npy + npz cells and fractions, up to 512 nz partial sums).  Asynchronous.
 * fb_grid_catalogue: out T[nx][ny][nz] = np.histogramdd(pos, bins=(nx, ny, nz), range=..., weights=weights) for the edge tables
 *   edges_x[nx + 1], edges_y[ny + 1], edges_z[nz + 1] (DEVICE double, non-decreasing: the caller's np.linspace(lo, hi, n + 1), so
 *   that the device compares with the same doubles as numpy).  pos: DEVICE double[n][3]; weights: DEVICE double[n] or NULL
 *   (all 1).  Bin = searchsorted(edges, p, 'right') - 1, a point equal to the last edge in the last bin; a point outside
 *   [edges[0], edges[n]] or NaN on any axis is dropped.  Not periodic.  Accumulated in fb_paint's fixed point (int64 with
 *   F = 61 - e, sum |w| < 2^e over all n particles; two words and 32 more bits on fp64 plans): the same bit for bit from call
 *   to call and for any particle order; unweighted counts are exact integers up to what T holds (2^24 per cell on a
 *   single-precision plan, 2^53 on fp64), at most 2^31 particles per cell.  The accumulators (8 or 16 bytes per cell) are
 *   plan-owned: FB_ERR_NOMEM if they do not fit.  Asynchronous.
 * fb_position_range: lohi6 (HOST) = {min x, max x, min y, max y, min z, max z} of pos (DEVICE double[n][3], n >= 1); both
 *   values of an axis are NaN if one of its coordinates is (numpy's min / max), infinities as they come.  Synchronises.     */
int fb_regrid_trilinear(fb_plan* plan, const void* cube, int nx, int ny, int nz, const double* gx, const double* gy,
                        const double* gz, const double* px, int npx, const double* py, int npy, const double* pz, int npz,
                        int swap_xy, void* out, void* stream);
int fb_grid_catalogue(fb_plan* plan, const double* pos, const double* weights, int64_t n, const double* edges_x, int nx,
                      const double* edges_y, int ny, const double* edges_z, int nz, void* out, void* stream);
int fb_position_range(fb_plan* plan, const double* pos, int64_t n, double* lohi6, void* stream);

/* ---- density-field (BAO) reconstruction and mesh readout (definition in DESIGN.md section 4; numpy statement in
 * tests/recon_numpy.py) ---------------------------------------------------------------------------------------------------
 * One box on one GPU, any box shape (Lx, Ly, Lz), both precisions, every grid the FFT takes.  Particle data are fp64 whatever
 * the plan's precision: pos DEVICE double[n][3] in Mpc, 0 <= n <= 2^31 - 2.  All arithmetic is fp64; fields are read and
 * written in the plan's precision.  The line of sight is z.  Everything here is asynchronous.
 * fb_recon_displacement: psi3_out T[3][N^3] = c2r(Psi_a(k)), a = x, y, z, with
 *     Psi_a(k) = i k_a delta(k) exp(-k^2 R^2 / 2) / (b (k^2 + beta k_z^2)),   k_a = 2 pi m_a / L_a, m_a the signed FFT index,
 *   the plane-parallel solution of div Psi + beta d_z Psi_z = -delta_smoothed / b for an irrotational Psi (beta = f / b;
 *   beta = 0: the Zel'dovich displacement of delta / b).  Zero at k = 0; component a is zero on the plane m_a = -N/2 (the
 *   convention of fb_cola_lpt; the stored k_z = N/2 plane of a half spectrum is that plane).  half_in: delta(k), a half
 *   spectrum (fb_fft_r2c), read once and kept; half_work3: scratch of three half spectra; the c2r scale is 1 / N^3.
 *   R > 0 (Mpc), b > 0, beta >= 0.
 * fb_mesh_readout: out DEVICE double[n][nfields] = sum over the window's nodes of w F_c at each position, for nfields (1..3)
 *   real fields T[nfields][N^3]; window, nodes and weights exactly fb_paint's (the readout is the adjoint of the paint), the
 *   weight of a node ((w_x w_y) w_z), nodes summed with x outermost.  Positions are periodic: the nodes wrap, whatever the
 *   position holds (|x| < 2^52 L); a position that is not finite reads NaN.  No atomics: bitwise repeatable.
 * fb_recon_shift: pos_out = wrap(x - scale Psi(x) - scale_z Psi_z(x) z^), Psi(x) the readout of psi3 T[3][N^3] at x:
 *   per axis wrap(x_a - scale Psi_a), along z wrap(x_z - (scale Psi_z + scale_z Psi_z)); wrap(x) = x - L floor(x / L), then
 *   + L if negative and - L if >= L.  pos_out may be pos_in.  A position that is not finite gives NaN on all three axes.
 *   For n >= N^3 / 8 the three fields are first copied interleaved (x, y, z, pad per node) into the plan's shared work buffer
 *   (4 N^3 reals) and gathered from there, one load per node: the same sums, the same bits.
 * fb_uniform_positions: n points uniform in the box from Philox stream 10.  Point p takes calls 2 p and 2 p + 1 of the stream
 *   (one call holds 128 bits, three 53-bit uniforms need 159): x from words (0, 1) and y from words (2, 3) of call 2 p, z from
 *   words (0, 1) of call 2 p + 1; u = (w + 1/2) 2^-53 with w = (a << 21) | (b >> 11); the coordinate is min(u L_a, the largest
 *   double below L_a).  Host model: fastbox_amd/rng.py recon_uniforms, bit for bit.
 * fb_grid_positions: pos_out DEVICE double[N^3][3] = one particle on each mesh node in C order, node m at m L_a / N (the
 *   randoms without shot noise); N^3 <= 2^31 - 2.
 * fb_recon_work_bytes: the device bytes CosmoBox.reconstruct allocates beside its inputs for n_data and n_random particles
 *   (eleven real fields, four half spectra, the shifted catalogues and fb_paint's accumulators); -1: bad arguments.         */
int64_t fb_recon_work_bytes(const fb_plan* plan, int64_t n_data, int64_t n_random);
int fb_recon_displacement(fb_plan* plan, const void* half_in, void* half_work3, void* psi3_out, double R, double b, double beta,
                          void* stream);
int fb_mesh_readout(fb_plan* plan, const void* fields, int nfields, const double* pos, int64_t n, int window, double* out,
                    void* stream);
int fb_recon_shift(fb_plan* plan, const void* psi3, const double* pos_in, int64_t n, int window, double scale, double scale_z,
                   double* pos_out, void* stream);
int fb_uniform_positions(fb_plan* plan, uint64_t seed, uint64_t realisation, int64_t n, double* pos_out, void* stream);
int fb_grid_positions(fb_plan* plan, double* pos_out, void* stream);

/* ---- Minkowski functionals of excursion sets (fb_minkowski.hip; definition: DESIGN.md section 4, numpy statement:
 * tests/minkowski_numpy.py).  real: T[N][N][N], periodic.  A voxel is a closed cell; an element of the cell complex (cell, face,
 * edge, vertex) lies in the excursion set of threshold t iff the maximum of its adjacent voxels (1, 2, 4, 8 of them) is >= t,
 * compared in fp64 on the stored value.  A NaN is below every threshold and is counted in n_nan_out; +inf is above every one.
 * thresholds: HOST double, 1 <= nt <= 256, finite and strictly ascending (per row), else FB_ERR_INVALID before any launch.
 *   mode 0: the box.  thresholds[nt]; counts_out HOST uint64 [8][nt] in the order n3, n2x, n2y, n2z, n1x, n1y, n1z, n0 (a face
 *     is named by its normal, an edge by the axis it runs along); n_nan_out HOST uint64 [1].
 *   mode 1: every channel z as a periodic 2-D map.  thresholds[nt]; counts_out [4][N][nt] in the order n2 (pixels), n1x, n1y
 *     (edges along x, y: 2 pixels each), n0 (vertices: 4 pixels); n_nan_out [N].
 *   mode 2: as mode 1 with thresholds[N][nt], a row per channel.
 * One pass over the cube; integer accumulation only (32-bit per workgroup in LDS, 64-bit device totals), so the counts are
 * exact and the same on every call.  Work memory: the thresholds and the histograms, in the plan's shared work buffer.
 * Synchronises.
 * fb_channel_moments: out_dev DEVICE double [2][N] = sum over the N^2 pixels of (v - mean_dev[c]) and of (v - mean_dev[c])^2 per
 * channel c, fp64 in a fixed order (the same bits on every call); mean_dev DEVICE double [N] as fb_channel_means writes it. */
int fb_minkowski_counts(fb_plan* plan, const void* real, const double* thresholds, int nt, int mode, uint64_t* counts_out,
                        uint64_t* n_nan_out, void* stream);
int fb_channel_moments(fb_plan* plan, const void* cube, const double* mean_dev, double* out_dev, void* stream);

/* ---- cosmic-web classification: tidal and shear tensors, their eigenvalues and classes (fb_web.hip; definition: DESIGN.md
 * section 4, numpy statement: tests/web_numpy.py).  One box on one GPU, any box shape, both precisions, every grid the FFT
 * takes.  Components are in the order xx, yy, zz, xy, xz, yz; pointer arrays are HOST arrays of DEVICE pointers.  With m_a the
 * signed FFT index (N/2 -> -N/2), k_a = 2 pi m_a / L_a and fp64 multipliers on both plans:
 * fb_tidal_k: half_out6[c] = k_i k_j / k^2 exp(-k^2 R^2 / 2) delta(k) for the six pairs, from one read of half_in (a half
 *   spectrum, fb_fft_r2c; kept).  Zero at k = 0; for i != j zero where m_i = -N/2 or m_j = -N/2; the diagonal keeps its Nyquist
 *   planes.  fb_fft_c2r of each output with scale 1 / N^3 is the component cube.  R >= 0 (Mpc).
 * fb_shear_k: half_out6[c] = -(i / 2 H0) (k_i v_j(k) + k_j v_i(k)) exp(-k^2 R^2 / 2) from one read of the three velocity
 *   spectra half_vel3 (kept); the term k_i v_j is zero where m_i = -N/2.  H0 > 0 in the velocity's units per Mpc.
 *   Both: the six outputs are distinct buffers and none is an input, else FB_ERR_INVALID (pointers are compared for equality:
 *   buffers that overlap in part are the caller's to avoid).  Asynchronous.
 * fb_web_eigen: per voxel of the six real cubes comp6 (T[N^3] each) the eigenvalues lambda_1 >= lambda_2 >= lambda_3 by
 *   cyclic Jacobi in fp64 with a fixed number of sweeps (backward stable: |error| of the order of 2^-53 ||A||_F, equal
 *   eigenvalues included; no data-dependent loop), and for each of nt thresholds (HOST double, 0 <= nt <= FB_WEB_NT_MAX,
 *   finite and strictly ascending) the class = the number of eigenvalues > threshold, decided in fp64: 0 void, 1 sheet,
 *   2 filament, 3 knot.  A voxel with a component that is not finite -- or with finite components so near the largest double
 *   that the solve overflows -- has three NaN eigenvalues and class 255; it is counted in n_nan_out and in no class.  Outputs, each of which may be NULL: eig3 (HOST array of three DEVICE T[N^3], entries may be
 *   NULL) the eigenvalues rounded to T; classes DEVICE uint8[N^3] for threshold index class_at; counts_out HOST uint64 [nt][4];
 *   wsum_out HOST double [nt][4], the sums of weight (DEVICE T[N^3]; NULL: zeros) per class; n_nan_out HOST uint64.  Counts are
 *   integer sums; weight sums are fp64, per lane, then per workgroup, then over the workgroups, each in a fixed order: the
 *   same bits on every call.  Work memory: the plan's shared work buffer.  Synchronises if a HOST output is asked for.
 * fb_web_mask: real_out T[N^3] = 1 where classes (DEVICE uint8[N^3]) == kind (0 .. 3), else 0.  Asynchronous.              */
#define FB_WEB_NT_MAX 16
int fb_tidal_k(fb_plan* plan, const void* half_in, void* const* half_out6, double R, void* stream);
int fb_shear_k(fb_plan* plan, const void* const* half_vel3, void* const* half_out6, double R, double H0, void* stream);
int fb_web_eigen(fb_plan* plan, const void* const* comp6, const double* thresholds, int nt, int class_at, const void* weight,
                 void* const* eig3, uint8_t* classes, uint64_t* counts_out, double* wsum_out, uint64_t* n_nan_out, void* stream);
int fb_web_mask(fb_plan* plan, const uint8_t* classes, int kind, void* real_out, void* stream);

/* ---- the steps after the density-field path: foregrounds (fastbox/foregrounds.py:48-175) and radiometer
 * noise (fastbox/noise.py:25-75).  2-D maps are T[N][N] over (x, y); cubes T[N][N][N], frequency axis last. ---- */
/* realise_foreground_amp (:99-107): map_out = Re ifft2((re + i im) amp2d) + monopole.  amp2d = sqrt(C_ell) per
 * 2-D mode with the k_perp = 0 entry 0 (:83-103, evaluated on the host); re, im = the reference's np.random.normal
 * draws as device maps, or both NULL for the counter generator (stream 2).  work_cplx: complex T[N][N] scratch. */
int fb_sky_realise_map(fb_plan* plan, const void* amp2d, const void* re, const void* im, uint64_t seed,
                       double monopole, void* work_cplx, void* map_out, void* stream);
/* realise_spectral_index (:137-138): map_out = mean + std n; n = `unit` (device map of N(0,1) draws) or generator */
int fb_sky_normal_map(fb_plan* plan, const void* unit, uint64_t seed, double mean, double std, void* map_out,
                      void* stream);
/* scipy.ndimage.gaussian_filter(map, sigma, mode='wrap') (:113, :144) with the 2*radius+1 HOST weights scipy
 * forms (exp(-x^2 / 2 sigma^2) normalised, radius = int(4 sigma + 0.5)); in place, tmp = T[N][N] scratch           */
int fb_sky_gaussian_filter(fb_plan* plan, void* map_inout, void* tmp, const double* weights, int radius, void* stream);
/* construct_cube (:165-175): cube = amps[x,y] * ratio[z] ** alpha[x,y] (alpha NULL: ** alpha_scalar);
 * ratio = freqs / freq_ref, HOST double[N]                                                                      */
int fb_sky_foreground_cube(fb_plan* plan, const void* amps, const void* alpha, double alpha_scalar,
                           const double* ratio, void* cube_out, void* stream);
/* realise_radiometer_noise (noise.py:72-74): cube = n[x,y,z] * sigma[z]; sigma = HOST double[N] (radiometer rms per
 * channel, :53-69 on the host); n = `unit` (device cube of the reference's draws) or the generator (stream 4)      */
int fb_sky_noise_cube(fb_plan* plan, const double* sigma, const void* unit, uint64_t seed, void* cube_out,
                      void* stream);

/* ---- interferometer: uv coverage of a set of projected baselines per channel, and the weighting of a transformed cube
 * (fastbox_amd/interferometer.py).  N even; cubes are [N][N][N] with the frequency channel c last; mode
 * index i of a transverse axis stands for the signed mode i (i <= N/2) or i - N.
 * fb_uv_coverage: samples_dev DEVICE double [ns][2], projected baselines (bx, by) in metres; mult_dev DEVICE int32 [ns]
 *   multiplicities >= 1 (NULL: all 1); sx_dev, sy_dev DEVICE double [N], cells per metre in channel c.  For sample s and
 *   channel c, in fp64: a = rint(bx sx[c]), b = rint(by sy[c]) (one multiply, one round-half-to-even each); the sample is
 *   accepted iff |a| <= N/2 and |b| <= N/2, and then adds m to counts[a mod N][b mod N][c] and m to
 *   counts[-a mod N][-b mod N][c] (the conjugate visibility of a real sky; a self-conjugate cell receives 2 m).  counts_dev
 *   DEVICE int32 [N][N][N], zeroed first unless accumulate = 1; the caller keeps 2 sum(m) <= 2^31 - 1.  Integer atomic adds:
 *   the same bits on every call.  ns = 0 is legal.  Asynchronous.
 * fb_uv_channel_sums: out_dev DEVICE int64 [2][N]: out[0][c] = sum of counts[.][.][c], out[1][c] = the number of cells of
 *   channel c with a count > 0.  Integer sums.  Asynchronous.
 * fb_uv_weight: full_cube_inout (complex T[N][N][N]) [x][y][c] *= f(counts[x][y][c]) scale_dev[c]; f(S) = S (mode 0),
 *   [S > 0] (1) or sqrt(S) (2); scale_dev DEVICE double [N].  The factor f scale is formed in fp64; each component is
 *   multiplied by it in fp64 and rounded once to T.  Asynchronous.                                                          */
int fb_uv_coverage(fb_plan* plan, const double* samples_dev, const int32_t* mult_dev, int64_t ns, const double* sx_dev,
                   const double* sy_dev, int32_t* counts_dev, int accumulate, void* stream);
int fb_uv_channel_sums(fb_plan* plan, const int32_t* counts_dev, int64_t* out_dev, void* stream);
int fb_uv_weight(fb_plan* plan, void* full_cube_inout, const int32_t* counts_dev, int mode, const double* scale_dev,
                 void* stream);

/* ---- slab-decomposed 3-D FFT for one box spread over `nparts` GPUs (one process per GPU) ---------
 * Rank `part` owns x-planes [part*N/nparts, ...) of real fields (T[N/nparts][N][N]) and, in k space,
 * k_y rows [part*N/nparts, ...) of every x-plane: kslab = complex<T>[N][N/nparts][pitch].
 * A forward transform is: fb_slab_forward_local (z r2c + y pass on the x-slab,
 * complex<T>[N/nparts][rows][pitch]) -> fb_slab_pack -> ONE all-to-all of equal blocks (done by the
 * caller: RCCL / torch.distributed) -> the receive buffer IS the kslab -> fb_slab_x_pass or the
 * fused fb_slab_x_bin.  The inverse mirrors it: fb_slab_x_generate (or x_pass) -> all-to-all of the
 * kslab's contiguous x-blocks -> fb_slab_unpack -> fb_slab_inverse_local (y pass + z c2r, 1/N^3).
 * The noise of fb_slab_x_generate depends on global mode indices only: the field is the same for
 * every nparts.  Cubic boxes only (shell amplitude / threshold tables).                          */
int64_t fb_slab_half_bytes(const fb_plan* plan, int nparts);     /* x-slab half spectrum           */
int64_t fb_slab_kspace_bytes(const fb_plan* plan, int nparts);   /* kslab = all-to-all buffer size  */
int fb_slab_forward_local(fb_plan* plan, const void* real_local, void* half_local, int nparts, int pre_exp,
                          double* expsum_dev, void* stream);
int fb_slab_inverse_local(fb_plan* plan, void* half_local, void* real_local, int nparts, void* stream);
/* the same two with fb_slab_pack / fb_slab_unpack folded into the y pass (it writes / reads the exchange buffer
 * directly); needs nparts to divide the points each thread holds of a y line: 1, 2, 4, 8 ranks (16 at N = 2048) */
int fb_slab_forward_packed(fb_plan* plan, const void* real_local, void* half_local, void* sendbuf, int nparts,
                           int pre_exp, double* expsum_dev, void* stream);
int fb_slab_inverse_packed(fb_plan* plan, const void* recvbuf, void* half_local, void* real_local, int nparts,
                           void* stream);
/* fb_slab_inverse_packed followed by fb_slab_forward_packed of the field just made, with the two z passes as one:
 * real_local (this rank's x-slab of delta_x) is written once and never read back.  recvbuf and sendbuf may be
 * the same buffer only if it is not half_local (the y passes are out of place).                                   */
int fb_slab_turnaround(fb_plan* plan, const void* recvbuf, void* half_local, void* real_local, void* sendbuf,
                       int nparts, int pre_exp, double* expsum_dev, void* stream);
int fb_slab_pack(fb_plan* plan, const void* half_local, void* sendbuf, int nparts, void* stream);
int fb_slab_unpack(fb_plan* plan, const void* recvbuf, void* half_local, int nparts, void* stream);
int fb_slab_x_pass(fb_plan* plan, void* kslab, int nparts, int direction, void* stream);
int fb_slab_x_generate(fb_plan* plan, void* kslab, int nparts, int part, uint64_t seed, uint64_t realisation,
                       void* stream);
/* results_dev[2*nbins]: this rank's (sum |dk|^2, sum |dk|^4) per bin; all-reduce (sum) over ranks */
int fb_slab_x_bin(fb_plan* plan, void* kslab, int nparts, int part, double* results_dev, void* stream);

/* ---- the same transform a range of k_z columns at a time, so that the all-to-all of one chunk of the half spectrum runs
 * beside the passes of the next (the x and y passes never mix k_z columns; only the z pass needs whole rows).
 * The strided passes work on tiles of `tile_columns` adjacent k_z columns; a row of the half spectrum has `tiles_per_row`
 * of them (fb_slab_tile_geometry); a chunk is the tile range [tile0, tile0 + ntile).  A chunk of the k-space slab and of
 * an exchange buffer is an ARRAY OF ITS OWN with row pitch W = ntile * tile_columns:
 *     k-chunk        complex[N][N/nparts][W]                 (x-major; block q = x-planes of rank q: contiguous)
 *     exchange chunk complex[nparts][N/nparts][N/nparts][W]  ([rank][x][k_y in rank][k_z in chunk])
 * -- equal contiguous blocks per rank, which is what the collective moves.  The x-slab's half spectrum `half_local`
 * ([N/nparts][N+1][pitch]) keeps all columns in one array.
 *   realise_density : fb_slab_x_generate_chunk(c) -> all-to-all(c) -> fb_slab_y_inverse_chunk(c), all c; fb_slab_z_pass(0)
 *   P(k)            : fb_slab_z_pass(1) -> fb_slab_y_forward_chunk(c) -> all-to-all(c) -> fb_slab_x_bin_chunk(c), all c
 *   both in one     : ... fb_slab_y_inverse_chunk(c) all c; fb_slab_z_pass(2); fb_slab_y_forward_chunk(c) ...
 * Fields are bit-identical to the unchunked calls for any chunking.                                                  */
int fb_slab_tile_geometry(const fb_plan* plan, int* tile_columns, int* tiles_per_row);
int fb_slab_x_generate_chunk(fb_plan* plan, void* kchunk, int nparts, int part, uint64_t seed, uint64_t realisation,
                             int tile0, int ntile, void* stream);
int fb_slab_y_inverse_chunk(fb_plan* plan, const void* recv_chunk, void* half_local, int nparts, int tile0, int ntile,
                            void* stream);
int fb_slab_y_forward_chunk(fb_plan* plan, const void* half_local, void* send_chunk, int nparts, int tile0, int ntile,
                            void* stream);
/* which: 0 = half_local -> real_local (c2r, numpy's 1/N^3), 1 = real_local -> half_local (r2c; of exp(real - shift) when
 * pre_exp, expsum_dev[0] = this rank's sum of them), 2 = c2r, store the field, r2c of (exp of) it from registers        */
int fb_slab_z_pass(fb_plan* plan, void* half_local, void* real_local, int nparts, int which, int pre_exp,
                   double* expsum_dev, void* stream);
/* first / last: the first and the last chunk of a spectrum (any order in between); results_dev as fb_slab_x_bin, written by
 * the last call */
int fb_slab_x_bin_chunk(fb_plan* plan, void* kchunk, int nparts, int part, int tile0, int ntile, int first, int last,
                        double* results_dev, void* stream);

/* ---- one box over several GPUs: communicator (RCCL over xGMI) --------------------------------------------------
 * The collectives of the slab-decomposed transform -- the all-to-all of equal blocks between the x-slab and the k_y-slab
 * layout (ONE per transform: fastbox/box.py:187 ifftn, :193 / :736 fftn), the all-reduce of the 2 nbins + 1 bin sums
 * (box.py:741-764) and of a field maximum -- behind the C ABI, so that a consumer of libfastbox_hip.so needs neither
 * PyTorch nor an MPI to run one box over the GPUs of a node: one process (or thread) per GPU, each with its own plan.
 *     rank 0:      fb_comm_unique_id(id);  hand the 128 bytes to the other ranks (file, socket, MPI_Bcast, ...)
 *     every rank:  fb_comm_create(plan, world, rank, id);
 *     per transform (or per k_z chunk):  fb_slab_x_generate[_chunk] -> fb_slab_exchange_begin -> ... the passes of the next
 *                  chunk on the caller's stream ... -> fb_slab_exchange_wait -> fb_slab_y_inverse_chunk / _inverse_packed
 *     fb_allreduce_f64(plan, results_dev, 2 * nbins + 1, 0, stream);   fb_comm_destroy(plan)   (fb_plan_destroy does it too)
 * The exchange runs on a stream the communicator owns (event hand-off from and to the caller's stream: the host never
 * blocks, and the caller's stream keeps computing between begin and wait); at most 16 exchanges in flight.  librccl is
 * opened on the first of these calls (FASTBOX_RCCL_LIB overrides the name); failures are FB_ERR_RCCL with RCCL's own message.
 * world = 1 with id = NULL needs no RCCL at all (the block moves by a device copy); world = 1 WITH an id makes a real
 * one-rank RCCL communicator.  fastbox_amd.distributed.RcclComm / SlabBox(comm="rccl") drive it from Python (ctypes). */
int fb_comm_unique_id(void* id128);                                   /* 128 bytes out                              */
int fb_comm_create(fb_plan* plan, int world, int rank, const void* id128);
int fb_comm_destroy(fb_plan* plan);
int fb_comm_info(const fb_plan* plan, int* world, int* rank, int* rccl_version);   /* world 0: no communicator     */
/* block q of send (bytes_per_peer bytes) -> rank q; block q of recv <- rank q; send != recv; ordered after `stream` */
int fb_slab_exchange_begin(fb_plan* plan, const void* send, void* recv, int64_t bytes_per_peer, void* stream, int* ticket);
int fb_slab_exchange_wait(fb_plan* plan, int ticket, void* stream);   /* `stream` waits for that exchange           */
int fb_slab_exchange(fb_plan* plan, const void* send, void* recv, int64_t bytes_per_peer, void* stream);   /* begin + wait */
/* in place on the device, in stream order of `stream` (issued, like the exchanges, to the communicator's own stream between two
 * event hand-overs: every operation of a communicator goes to one stream, in the same order on every rank); op 0 = sum, 1 = max */
int fb_allreduce_f64(fb_plan* plan, double* data_dev, int count, int op, void* stream);

/* The y and z passes of a transform run x-plane batch by x-plane batch so that a batch stays in the 256 MiB Infinity
 * Cache between them.  planes = -1: sized for ONE box using the GPU (default); when several boxes run concurrently on
 * their own streams, give each its share (e.g. 64 planes of a 512^3 box for two).  0 = whole box in one go.
 * streams = 2 sends alternate batches to a second stream of the plan; 0 = by grid size. */
int fb_set_plane_batching(fb_plan* plan, int planes, int streams);
/* How the strided FFT passes (x, y) of this plan are scheduled, per class (plain pass, fused generator pass, fused
 * binning pass): 0 = one workgroup per tile, 1 = resident workgroups that walk the tiles and load their next tile
 * while finishing the current one, -1 (default) = by grid size (resident where a CU holds one workgroup of the pass: N = 2048, and the generator pass from N = 1024).  The transforms are bit-identical in both forms; the binning pass groups its fp64
 * partial sums by resident workgroup instead of by tile (differences at the 1e-16 level).  Grids below 256^3 always use 0. */
int fb_set_pass_schedule(fb_plan* plan, int plain, int generator, int binning);
/* Row segment of the strided passes' tiles where a plan has a choice -- single precision at N = 2048: 128 bytes = 2048 rows x 16
 * columns exchanged through LDS as real and imaginary halves, 32 points per thread; 64 bytes = 2048 rows x 8 columns, 16 points
 * per thread (the form of rounds 1-3, which the slab-decomposed path's k_z-chunk launches keep).  0 = the library's choice per
 * pass class (the plain passes wide, the fused generator and binning passes narrow: they need their registers for the parked
 * stores / the second tile).  Transforms are bit-identical in both forms (the same radix-8/8/8/4 stages); the binning pass groups
 * its single-precision partial sums differently (1e-9 relative on a bin). */
int fb_set_tile_rows(fb_plan* plan, int bytes);
/* Fused log-normal transforms (pre_exp of fb_fft_r2c / fb_power_spectrum_device / _pending) form exp(x - shift).  The
 * estimate exp(d)/mean(exp(d)) - 1 does not depend on the shift (results[2 nbins] is the sum of the SHIFTED exponentials,
 * which is what the caller normalises with); the right shift keeps a single-precision plan's sum of exponentials (the
 * k = 0 mode), its |delta_k|^2 and |delta_k|^4 sums inside the float range whatever the field's variance: about
 * ln(sum exp(d)) - 7, see fastbox_amd/hostgeom.py lognormal_shift (from the field's variance) and lognormal_shift_exact
 * (from fb_max_real). */
int fb_set_exp_shift(fb_plan* plan, double shift);
/* tuning aid: a single strided FFT pass over a half spectrum (axis 0 = x, 1 = y;
 * mode 0 plain in place, 1 fused generator, 2 fused binning without store) */
int fb_debug_strided_pass(fb_plan* plan, void* half, int axis, int mode, void* stream);
/* testing aid: the number of pair tests after which a workgroup of fb_pair_count's sweep flushes its 32-bit LDS histogram
 * to the global one (1 .. 2^31; 0: the default, 2^31, which no input of a few thousand points reaches).  Process-wide; the
 * counts do not depend on it. */
int fb_debug_pair_flush(int64_t pairs);
/* diagnostic builds (-DFB_STAMPS) only: per-workgroup phase time stamps of the last plain pass */
int fb_debug_read_stamps(fb_plan* plan, long long* host, int64_t count);

/* ---- device memory helpers for bindings without their own allocator ---------------------------- */
int fb_malloc(void** dev_ptr, size_t bytes);
int fb_free(void* dev_ptr);
int fb_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int fb_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int fb_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int fb_stream_create(void** stream);     /* a non-blocking hipStream_t, for running independent boxes concurrently */
int fb_stream_create_priority(void** stream, int priority);   /* priority < 0: the device's highest, 0: middle, > 0: lowest */
int fb_stream_destroy(void* stream);
int fb_stream_sync(void* stream);
/* work queued on `waiter` after this call starts only when everything queued on `signaller` before it has finished
 * (both streams on the current device); the host does not wait */
int fb_stream_wait_stream(void* waiter, void* signaller);
int fb_device_count(int* count);
/* The calling thread's current HIP device.  Every entry point that takes a plan makes the plan's device current for the
 * duration of the call and restores the caller's before it returns, so the library never moves the current device under
 * other users of the runtime (torch, RCCL).  The plan-less helpers above (fb_malloc, fb_stream_create,
 * fb_stream_wait_stream) act on the CURRENT device: a binding that serves a box on another device brackets them with
 * fb_device_get / fb_device_set / fb_device_set(previous), as fastbox_amd/_lib.py on_device() does. */
int fb_device_get(int* device);
int fb_device_set(int device);

#ifdef __cplusplus
}
#endif
#endif
