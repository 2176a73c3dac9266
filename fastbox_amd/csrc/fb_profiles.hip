// Radial profiles and aperture moments of the particles around given centres (the spherical-overdensity
// masses of halos.py are built on them): the particles are binned once into a grid of cells (fb_cells.h, shared with
// fb_fof.hip and fb_pairs.hip), then one workgroup per centre walks the particles of the distinct neighbour cells of the
// centre's cell and either counts them into the centre's own row of radial bins or sums the moments of those inside the
// centre's own radius.  Particle data are fp64 whatever the plan's precision; the plan gives the box and the device.  See
// include/fastbox_hip.h for the entry points.
//
// No contraction anywhere in this file: the wrapped positions, the minimum-image differences and
// d^2 = (dx dx + dy dy) + dz dz must be the doubles of the numpy statement (tests/profiles_numpy.py), so that a particle on
// an edge falls on the device into the bin it falls into there.  No square root is taken in any comparison.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_cells.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define FB_PROF_SMALL 256                // bytes at the head of the work buffer: the words of ProfSmall
#define FB_PROF_WG 256                   // threads per workgroup of the sweep
#define FB_PROF_MAX_NR 256
#define FB_PROF_HIST 4096                // words of the LDS histogram: (nr + 1) columns x interleaved copies
#define FB_PROF_MAGIC 0x6b0f11e5u        // the work buffer has been prepared by fb_profile_bin
#define FB_PROF_ERR_REACH 8u             // error word (1 and 4 are FB_FOF_ERR_POS, FB_FOF_ERR_VEL): an aperture beyond the reach
#define FB_PROF_NACC 14                  // two words for each of 3 offsets, 3 velocities and v.v

namespace {

// what fb_profile_bin leaves for the sweeps, and the error word of every call
struct ProfSmall {
    unsigned err, magic;
    int with_vel, nc[3];
    unsigned long long n, ncells, vmax_bits;
};
static_assert(sizeof(ProfSmall) <= FB_PROF_SMALL, "ProfSmall");

struct ProfBins { int nr, rsteps, copies_log2; };
struct ProfFix { int Fp, Fv, Fvv; };     // fractional bits of the offset, velocity and v.v sums

// svel[slot] = vel[perm[slot]]: the velocities in the order of the permuted positions, so that the sweep reads both alike
__global__ __launch_bounds__(256) void k_prof_gather(const double* vel, const unsigned* perm, unsigned long long n, double* svel) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256) {
        const unsigned long long i = perm[q];
        svel[3 * q] = vel[3 * i]; svel[3 * q + 1] = vel[3 * i + 1]; svel[3 * q + 2] = vel[3 * i + 2];
    }
}

__device__ __forceinline__ void fx_acc(unsigned long long* a, double x, int F) {
    unsigned long long hi, lo;
    fx_split(ldexp(x, F), hi, lo);
    a[0] += hi;
    a[1] += lo;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup per centre, grid-stride over the centres.  The centre is wrapped and its cell found as a particle's is; the
// distinct neighbour cells are walked once each: an offset of -1 along an axis of fewer than 3 cells names the cell of +1 and
// is skipped, and along z, where adjacent cells are contiguous in the sorted array, the column of up to three cells is one
// range of slots, or two where it crosses the seam.  Thread t takes slots q0 + t, q0 + t + 256, ... of a range: every loop
// is bounded by a cell's occupancy or a constant.  A particle is decided by its own minimum-image differences.
//
// APERTURE false (profiles): column 0 of the centre's row counts d^2 < e2[0], column b + 1 counts e2[b] <= d^2 < e2[b + 1],
// b by bisection over e2 in LDS; the count goes to copy (lane mod copies) of the workgroup's interleaved LDS histogram, as in
// k_pair_sweep.  A row sums to at most n < 2^31, so no 32-bit counter wraps.  The workgroup owns the row and writes it with
// plain stores: no global atomic.
// APERTURE true: the particles with d^2 < r2[h] are counted and their offsets d, their velocities and v.v = (vx vx + vy vy)
// + vz vz summed in two-word fixed point (fb_dev.h) per thread, then over the wave and through LDS over the workgroup:
// integer adds, so any order gives the same words.  Thread 0 forms com = wrap(c + sum d / m), vmean = sum v / m and
// sigma = sqrt(max(0, (sum v.v / m - vmean.vmean) / 3)); m = 0: NaN.  r2[h] > reach2 (or NaN) sets FB_PROF_ERR_REACH.
// A centre that is not finite or has |x| >= 2^52 L sets FB_FOF_ERR_POS; its outputs are not written.
template <bool APERTURE>
__global__ __launch_bounds__(FB_PROF_WG) void k_centre_sweep(FofGeom g, const unsigned* start, const double* spos, const double* svel,
                                                            const double* centres, unsigned long long nh, const double* e2g,
                                                            ProfBins pb, unsigned* counts_out, const double* r2, double reach2,
                                                            ProfFix fx, unsigned* count_out, double* com_out, double* vmean_out,
                                                            double* sigma_out, unsigned* err) {
    __shared__ double e2[APERTURE ? 1 : FB_PROF_MAX_NR + 1];
    __shared__ unsigned hist[APERTURE ? 1 : FB_PROF_HIST];
    __shared__ unsigned long long red[APERTURE ? 4 * (FB_PROF_NACC + 1) : 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ncol = pb.nr + 1;
    const unsigned copy = (unsigned)lane & ((1u << pb.copies_log2) - 1u);
    double e2lo = 0.0, e2hi = 0.0;
    if constexpr (!APERTURE) {
        for (int i = t; i <= pb.nr; i += FB_PROF_WG) e2[i] = e2g[i];
        for (int i = t; i < (ncol << pb.copies_log2); i += FB_PROF_WG) hist[i] = 0u;
        __syncthreads();
        e2lo = e2[0]; e2hi = e2[pb.nr];
    }
    for (unsigned long long h = blockIdx.x; h < nh; h += gridDim.x) {
        const double x0 = centres[3 * h], x1 = centres[3 * h + 1], x2 = centres[3 * h + 2];
        const double w0 = wrap_pos(x0, g.L[0]), w1 = wrap_pos(x1, g.L[1]), w2 = wrap_pos(x2, g.L[2]);
        const bool small = fabs(x0) < FB_FOF_WRAP_MAX * g.L[0] && fabs(x1) < FB_FOF_WRAP_MAX * g.L[1] && fabs(x2) < FB_FOF_WRAP_MAX * g.L[2];
        if (!(small && w0 >= 0.0 && w0 < g.L[0] && w1 >= 0.0 && w1 < g.L[1] && w2 >= 0.0 && w2 < g.L[2])) {     // the same in every thread
            if (t == 0) atomicOr(err, FB_FOF_ERR_POS);
            continue;
        }
        double lim2 = e2hi;
        if constexpr (APERTURE) {
            lim2 = r2[h];
            if (!(lim2 <= reach2)) {
                if (t == 0) atomicOr(err, FB_PROF_ERR_REACH);
                continue;
            }
        }
        const unsigned c = fof_cell(g, w0, w1, w2);
        const int c2 = (int)(c % (unsigned)g.nc[2]), c1 = (int)((c / (unsigned)g.nc[2]) % (unsigned)g.nc[1]),
                  c0 = (int)(c / ((unsigned)g.nc[2] * (unsigned)g.nc[1]));
        // the column c2 - 1 .. c2 + 1 as ranges [zlo, zhi) of cells along z
        int nrange = 1, zlo[2] = {0, 0}, zhi[2] = {g.nc[2], 0};
        if (g.nc[2] > 3) {
            if (c2 == 0) { nrange = 2; zlo[0] = 0; zhi[0] = 2; zlo[1] = g.nc[2] - 1; zhi[1] = g.nc[2]; }
            else if (c2 == g.nc[2] - 1) { nrange = 2; zlo[0] = c2 - 1; zhi[0] = g.nc[2]; zlo[1] = 0; zhi[1] = 1; }
            else { zlo[0] = c2 - 1; zhi[0] = c2 + 2; }
        }
        unsigned cnt = 0;
        unsigned long long acc[APERTURE ? FB_PROF_NACC : 1];
        if constexpr (APERTURE) {
#pragma unroll
            for (int k = 0; k < FB_PROF_NACC; ++k) acc[k] = 0ull;
        }
        for (int o0 = g.nc[0] < 3 ? 0 : -1; o0 <= 1; ++o0) {
            const int m0 = (c0 + o0 + g.nc[0]) % g.nc[0];
            for (int o1 = g.nc[1] < 3 ? 0 : -1; o1 <= 1; ++o1) {
                const int m1 = (c1 + o1 + g.nc[1]) % g.nc[1];
                const unsigned base = ((unsigned)m0 * (unsigned)g.nc[1] + (unsigned)m1) * (unsigned)g.nc[2];
                for (int r = 0; r < nrange; ++r) {
                    const unsigned q1 = start[base + (unsigned)zhi[r]];
                    for (unsigned q = start[base + (unsigned)zlo[r]] + (unsigned)t; q < q1; q += FB_PROF_WG) {
                        const double dx = fof_min_image(spos[3ull * q] - w0, g.L[0]), dy = fof_min_image(spos[3ull * q + 1] - w1, g.L[1]),
                                     dz = fof_min_image(spos[3ull * q + 2] - w2, g.L[2]);
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(d2 < lim2)) continue;
                        if constexpr (APERTURE) {
                            ++cnt;
                            fx_acc(acc, dx, fx.Fp); fx_acc(acc + 2, dy, fx.Fp); fx_acc(acc + 4, dz, fx.Fp);
                            if (svel) {
                                const double vx = svel[3ull * q], vy = svel[3ull * q + 1], vz = svel[3ull * q + 2];
                                fx_acc(acc + 6, vx, fx.Fv); fx_acc(acc + 8, vy, fx.Fv); fx_acc(acc + 10, vz, fx.Fv);
                                fx_acc(acc + 12, (vx * vx + vy * vy) + vz * vz, fx.Fvv);
                            }
                        } else {
                            int col = 0;
                            if (d2 >= e2lo) {
                                int lo = 0, hi = pb.nr - 1;                   // the largest b with e2[b] <= d2
                                for (int s = 0; s < pb.rsteps; ++s) {
                                    const int mid = (lo + hi + 1) >> 1;
                                    if (e2[mid] <= d2) lo = mid; else hi = mid - 1;
                                }
                                col = lo + 1;
                            }
                            atomicAdd(&hist[((unsigned)col << pb.copies_log2) + copy], 1u);
                        }
                    }
                }
            }
        }
        if constexpr (APERTURE) {
#pragma unroll
            for (int k = 0; k < FB_PROF_NACC; ++k) acc[k] = wave_sum_u64(acc[k]);
            const unsigned long long wc = wave_sum_u64((unsigned long long)cnt);
            __syncthreads();                                          // thread 0 has read red of the previous centre
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < FB_PROF_NACC; ++k) red[wave * (FB_PROF_NACC + 1) + k] = acc[k];
                red[wave * (FB_PROF_NACC + 1) + FB_PROF_NACC] = wc;
            }
            __syncthreads();
            if (t == 0) {
                unsigned long long tot[FB_PROF_NACC + 1];
#pragma unroll
                for (int k = 0; k <= FB_PROF_NACC; ++k)
                    tot[k] = (red[k] + red[(FB_PROF_NACC + 1) + k]) + (red[2 * (FB_PROF_NACC + 1) + k] + red[3 * (FB_PROF_NACC + 1) + k]);
                const unsigned long long m = tot[FB_PROF_NACC];
                const double md = (double)m, w[3] = {w0, w1, w2};
                count_out[h] = (unsigned)m;
                double vv = 0.0, vm[3] = {0.0, 0.0, 0.0};
                for (int a = 0; a < 3; ++a) {
                    com_out[3 * h + a] = m ? wrap_pos(w[a] + fx_join(tot[2 * a], tot[2 * a + 1], fx.Fp) / md, g.L[a]) : NAN;
                    if (vmean_out) {
                        vm[a] = m ? fx_join(tot[6 + 2 * a], tot[7 + 2 * a], fx.Fv) / md : NAN;
                        vmean_out[3 * h + a] = vm[a];
                    }
                }
                if (sigma_out) {
                    vv = (vm[0] * vm[0] + vm[1] * vm[1]) + vm[2] * vm[2];
                    sigma_out[h] = m ? sqrt(fmax(0.0, (fx_join(tot[12], tot[13], fx.Fvv) / md - vv) / 3.0)) : NAN;
                }
            }
        } else {
            __syncthreads();
            const int nc = 1 << pb.copies_log2;
            for (int b = t; b < ncol; b += FB_PROF_WG) {
                unsigned sum = 0;
                for (int q = 0; q < nc; ++q) {
                    const int w = (b << pb.copies_log2) + ((q + b) & (nc - 1));   // start at copy b: a wave's threads on different banks
                    sum += hist[w];
                    hist[w] = 0u;
                }
                counts_out[h * (unsigned long long)ncol + (unsigned long long)b] = sum;
            }
            __syncthreads();                                          // the histogram is clear before the next centre adds to it
        }
    }
}

int prof_ceil_log2(int n) {
    int s = 0;
    while ((1 << s) < n) ++s;
    return s;
}

// the work buffer: small | e2 f64[257] | spos f64[3 n] | svel f64[3 n] (with_vel) | start u32[ncells + 1] | cursor u32[ncells] |
// csum u32[chunks] | cellid u32[n] | perm u32[n] (with_vel)
struct ProfWork { size_t e2, spos, svel, start, cursor, csum, cellid, perm, total; };
ProfWork prof_layout(unsigned long long n, unsigned long long ncells, bool with_vel) {
    ProfWork w;
    size_t o = FB_PROF_SMALL;
    w.e2 = o; o += align16((size_t)(FB_PROF_MAX_NR + 1) * 8);
    w.spos = o; o += align16((size_t)n * 24);
    w.svel = o; o += with_vel ? align16((size_t)n * 24) : 0;
    w.start = o; o += align16((size_t)(ncells + 1) * 4);
    w.cursor = o; o += align16((size_t)ncells * 4);
    w.csum = o; o += align16((size_t)scan_chunks(ncells) * 4);
    w.cellid = o; o += align16((size_t)n * 4);
    w.perm = o; o += with_vel ? align16((size_t)n * 4) : 0;
    w.total = o;
    return w;
}

// the header of a prepared work buffer, checked; *g, *w: the geometry and layout it was prepared with
int prof_open(fb_plan* p, const void* work, hipStream_t s, ProfSmall* h, FofGeom* g, ProfWork* w) {
    FB_TRY(fb_read_back(h, work, sizeof(*h), s));
    FB_REQUIRE(h->magic == FB_PROF_MAGIC, "profiles: the work buffer has not been prepared by fb_profile_bin");
    *g = geom_of(p, h->nc);
    *w = prof_layout(h->n, h->ncells, h->with_vel != 0);
    return FB_OK;
}
// a reach of reach2 (squared) inside the cells of a prepared work buffer
bool prof_reach_fits(const fb_plan* p, const ProfSmall& h, double reach2) {
    for (int a = 0; a < 3; ++a) {
        const double side = p->L[a] / (double)h.nc[a];
        if (!(reach2 < 0.25 * p->L[a] * p->L[a] && side * side >= reach2)) return false;
    }
    return true;
}
unsigned prof_grid(const fb_plan* p, int64_t nh) {
    return (unsigned)std::min<unsigned long long>((unsigned long long)nh, 8ull * (unsigned long long)p->num_cu);
}

}  // namespace

extern "C" {

int64_t fb_profile_work_bytes(int64_t n, int64_t ncells, int with_vel) {
    if (n < 0 || ncells < 1) return -1;
    return (int64_t)prof_layout((unsigned long long)n, (unsigned long long)ncells, with_vel != 0).total;
}

int fb_profile_bin(fb_plan* p, const double* pos, int64_t n, const double* vel, const int* ncell, void* work, int64_t work_bytes,
                   int* bad, double* stage_ms, void* stream) {
    FB_REQUIRE(p && ncell && work && bad, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll, "profiles: 0 <= n <= 2^31 - 2");
    unsigned long long ncells = 1;
    for (int a = 0; a < 3; ++a) {
        FB_REQUIRE(ncell[a] >= 2, "profiles: at least 2 cells per axis");
        ncells *= (unsigned long long)ncell[a];
        FB_REQUIRE(ncells <= (1ull << 31), "profiles: at most 2^31 cells");
    }
    const bool with_vel = vel != nullptr;
    const ProfWork w = prof_layout((unsigned long long)n, ncells, with_vel);
    FB_REQUIRE(work_bytes >= (int64_t)w.total, "profiles: work buffer smaller than fb_profile_work_bytes");
    FB_REQUIRE(n == 0 || pos, "null pointer");
    *bad = 0;
    if (stage_ms) stage_ms[0] = 0.0;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    char* wb = (char*)work;
    ProfSmall* sm = (ProfSmall*)wb;
    double *spos = (double*)(wb + w.spos), *svel = (double*)(wb + w.svel);
    unsigned *start = (unsigned*)(wb + w.start), *cursor = (unsigned*)(wb + w.cursor), *csum = (unsigned*)(wb + w.csum),
             *cellid = (unsigned*)(wb + w.cellid), *perm = with_vel ? (unsigned*)(wb + w.perm) : nullptr;
    const FofGeom g = geom_of(p, ncell);
    const unsigned long long un = (unsigned long long)n;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (stage_ms) for (int q = 0; q < 2; ++q) FB_HIP(hipEventCreate(&ev[q]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int q = 0; q < 2; ++q) if (e[q]) (void)hipEventDestroy(e[q]); } } evg{ev};
    if (stage_ms) FB_HIP(hipEventRecord(ev[0], s));
    FB_HIP(hipMemsetAsync(sm, 0, FB_PROF_SMALL, s));                 // magic 0: not prepared until the end of this call
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_bin, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, cellid, cursor, &sm->err);
    FB_LAUNCH_CHECK("k_fof_bin");
    if (with_vel) {
        hipLaunchKernelGGL(k_fof_vmax, dim3(grid_for(3 * un, p)), dim3(256), 0, s, vel, 3 * un, &sm->vmax_bits, &sm->err);
        FB_LAUNCH_CHECK("k_fof_vmax");
    }
    ProfSmall h;
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    if (h.err & FB_FOF_ERR_POS) { *bad = 1; return FB_OK; }          // before anything is prepared
    double vmax;
    memcpy(&vmax, &h.vmax_bits, sizeof(vmax));
    if ((h.err & FB_FOF_ERR_VEL) || !std::isfinite(3.0 * (double)n * vmax * vmax)) { *bad = 4; return FB_OK; }   // the sums' bound
    FB_TRY(exscan(ScanPlain{cursor}, ncells, csum, start, s));       // start[ncells] = n
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_scatter, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, (const unsigned*)cellid, (const unsigned*)start,
                       cursor, perm, spos, (unsigned*)nullptr);
    FB_LAUNCH_CHECK("k_fof_scatter");
    if (with_vel) {
        hipLaunchKernelGGL(k_prof_gather, dim3(grid_for(un, p)), dim3(256), 0, s, vel, (const unsigned*)perm, un, svel);
        FB_LAUNCH_CHECK("k_prof_gather");
    }
    h.err = 0; h.magic = FB_PROF_MAGIC; h.with_vel = with_vel ? 1 : 0;
    for (int a = 0; a < 3; ++a) h.nc[a] = ncell[a];
    h.n = un; h.ncells = ncells;
    FB_HIP(hipMemcpyAsync(sm, &h, sizeof(h), hipMemcpyHostToDevice, s));
    if (stage_ms) FB_HIP(hipEventRecord(ev[1], s));
    FB_HIP(hipStreamSynchronize(s));                                  // h lives on this stack
    if (stage_ms) {
        float ms = 0.f;
        FB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stage_ms[0] = (double)ms;
    }
    return FB_OK;
}

int fb_halo_profiles(fb_plan* p, void* work, const double* centres, int64_t nh, const double* edges2, int nr, uint32_t* counts_out,
                     int* bad, void* stream) {
    FB_REQUIRE(p && work && edges2 && bad, "null pointer");
    FB_REQUIRE(nh >= 0 && nh <= 2147483646ll, "profiles: 0 <= nh <= 2^31 - 2");
    FB_REQUIRE(nr >= 1 && nr <= FB_PROF_MAX_NR, "profiles: 1 <= nr <= 256");
    FB_REQUIRE(edges2[0] >= 0.0, "profiles: edges[0] >= 0");
    for (int b = 0; b < nr; ++b) FB_REQUIRE(edges2[b] < edges2[b + 1], "profiles: strictly ascending edges");   // NaN fails
    FB_REQUIRE(nh == 0 || (centres && counts_out), "null pointer");
    *bad = 0;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    ProfSmall h;
    FofGeom g;
    ProfWork w;
    FB_TRY(prof_open(p, work, s, &h, &g, &w));
    FB_REQUIRE(prof_reach_fits(p, h, edges2[nr]), "profiles: the last edge must stay below L / 2 and within the side of the binned cells");
    if (nh == 0) return FB_OK;
    char* wb = (char*)work;
    ProfSmall* sm = (ProfSmall*)wb;
    double* e2d = (double*)(wb + w.e2);
    FB_HIP(hipMemsetAsync(&sm->err, 0, sizeof(unsigned), s));
    FB_HIP(hipMemcpyAsync(e2d, edges2, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, s));
    ProfBins pb;
    pb.nr = nr; pb.rsteps = prof_ceil_log2(nr); pb.copies_log2 = 0;
    while (pb.copies_log2 < 6 && ((nr + 1) << (pb.copies_log2 + 1)) <= FB_PROF_HIST) ++pb.copies_log2;
    hipLaunchKernelGGL(k_centre_sweep<false>, dim3(prof_grid(p, nh)), dim3(FB_PROF_WG), 0, s, g, (const unsigned*)(wb + w.start),
                       (const double*)(wb + w.spos), (const double*)nullptr, centres, (unsigned long long)nh, (const double*)e2d, pb,
                       (unsigned*)counts_out, (const double*)nullptr, 0.0, ProfFix{0, 0, 0}, (unsigned*)nullptr, (double*)nullptr,
                       (double*)nullptr, (double*)nullptr, &sm->err);
    FB_LAUNCH_CHECK("k_centre_sweep");
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));   // (the edges have been read by now, too)
    *bad = (int)h.err;
    return FB_OK;
}

int fb_halo_apertures(fb_plan* p, void* work, const double* centres, const double* r2, int64_t nh, double reach, uint32_t* count_out,
                      double* com_out, double* vmean_out, double* sigma_out, int* bad, void* stream) {
    FB_REQUIRE(p && work && bad, "null pointer");
    FB_REQUIRE(nh >= 0 && nh <= 2147483646ll, "profiles: 0 <= nh <= 2^31 - 2");
    FB_REQUIRE(reach >= 0.0 && std::isfinite(reach), "profiles: a finite reach >= 0");
    FB_REQUIRE(nh == 0 || (centres && r2 && count_out && com_out), "null pointer");
    FB_REQUIRE((vmean_out == nullptr) == (sigma_out == nullptr), "profiles: vmean_out and sigma_out together, or neither");
    *bad = 0;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    ProfSmall h;
    FofGeom g;
    ProfWork w;
    FB_TRY(prof_open(p, work, s, &h, &g, &w));
    FB_REQUIRE(prof_reach_fits(p, h, reach * reach), "profiles: the reach must stay below L / 2 and within the side of the binned cells");
    FB_REQUIRE(!vmean_out || h.with_vel, "profiles: velocity moments need a work buffer binned with velocities");
    if (nh == 0) return FB_OK;
    char* wb = (char*)work;
    ProfSmall* sm = (ProfSmall*)wb;
    // every |sum| stays below 2^e: at most n terms, each offset below max(L) / 2, each |v| at most vmax, each v.v at most 3 vmax^2
    double vmax;
    memcpy(&vmax, &h.vmax_bits, sizeof(vmax));
    const double nd = (double)h.n;
    auto bits = [](double bound) { int e = 0; if (bound > 0.0) (void)frexp(bound, &e); return 93 - e; };
    const ProfFix fx{bits(nd * 0.5 * std::max(p->L[0], std::max(p->L[1], p->L[2]))), bits(nd * vmax), bits(3.0 * nd * vmax * vmax)};
    FB_HIP(hipMemsetAsync(&sm->err, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_centre_sweep<true>, dim3(prof_grid(p, nh)), dim3(FB_PROF_WG), 0, s, g, (const unsigned*)(wb + w.start),
                       (const double*)(wb + w.spos), vmean_out ? (const double*)(wb + w.svel) : (const double*)nullptr, centres,
                       (unsigned long long)nh, (const double*)nullptr, ProfBins{1, 0, 0}, (unsigned*)nullptr, r2, reach * reach, fx,
                       (unsigned*)count_out, com_out, vmean_out, sigma_out, &sm->err);
    FB_LAUNCH_CHECK("k_centre_sweep");
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    *bad = (int)h.err;
    return FB_OK;
}

}  // extern "C"
