// Three-point correlation multipoles of a weighted catalogue in the periodic box (Slepian & Eisenstein 2015; DESIGN.md
// section 4): the particles are binned once into a grid of cells (fb_cells.h, shared with fb_fof.hip, fb_pairs.hip and
// fb_profiles.hip), then one workgroup per primary walks the particles of the distinct neighbour cells of the primary's cell
// as k_centre_sweep of fb_profiles.hip does, sums the real spherical harmonics of the directions to its neighbours per radial
// bin, a_lm(b), and contracts them pairwise into the primary's share of M_l(b1, b2).  Particle data are fp64 whatever the
// plan's precision; the plan gives the box and the device.  See include/fastbox_hip.h for the definition and the entry points.
//
// No contraction anywhere in this file: the wrapped positions, the minimum-image differences, d^2 = (dx dx + dy dy) + dz dz
// and every step of the harmonic recurrence must be the doubles of the numpy statement (tests/threepoint_numpy.py).  Every sum
// over particles is fixed-point in two 64-bit words (fb_dev.h): integer adds, so the results are the same bit for bit from
// call to call and for any order of the particles.  No float atomic anywhere.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_cells.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define FB_TRIP_SMALL 256                // bytes at the head of the work buffer: the words of TripSmall
#define FB_TRIP_WG_SMALL 256             // threads per workgroup of the sweep for tables of up to 64 rows (lmax <= 6)
#define FB_TRIP_WG_LARGE 512             // and beyond: phase C is then a long chain per thread, and a second wave per SIMD hides its LDS latency
#define FB_TRIP_MAX_NW (FB_TRIP_WG_LARGE / 64)
#define FB_TRIP_MAX_NR 32
#define FB_TRIP_MAX_L 10
#define FB_TRIP_MAX_PROBE 64
#define FB_TRIP_MAX_WG 512               // workgroups of the sweep at most: each has its own partial sums of M
#define FB_TRIP_TILE 64                  // in-range neighbours per tile
#define FB_TRIP_YS 65                    // doubles per row of the tile of harmonics: 64 and one of padding
#define FB_TRIP_STAGE(wg) (64 + (wg))    // staged neighbours at most: fewer than a tile left over and one stride of the workgroup
#define FB_TRIP_LDS_MAX 163840           // the CU's 160 KiB
// the table of constants, in doubles: A_m | sqrt(2 m + 3) | alpha_lm | beta_lm | 4 pi / (2 l + 1) | sqrt(2)
#define FB_TRIP_NT 11
#define FB_TRIP_TAB_A 0
#define FB_TRIP_TAB_G 11
#define FB_TRIP_TAB_AL 22
#define FB_TRIP_TAB_BE 143
#define FB_TRIP_TAB_FL 264
#define FB_TRIP_TAB_SQ2 275
#define FB_TRIP_TAB 276

namespace {

struct TripSmall {
    unsigned err, pad;
    unsigned long long wmax_bits;
};
static_assert(sizeof(TripSmall) <= FB_TRIP_SMALL, "TripSmall");

// byte offsets into the dynamic LDS of the sweep, every one a multiple of 16
struct TripLds { int e2, tab, hi, lo, yt, ss, sx, sy, sz, sw, sb, cnt, pairb, wtot, probe, total; };

struct TripArgs {
    FofGeom g;
    unsigned long long n;
    int nr, rsteps, lmax, nlm, rows, nrp, parts, per, npair, nent, nprobe;
    int Fa, Fs, Fm;                      // fractional bits of the a_lm, the sum of w^2 and M
    TripLds o;
};

size_t trip_al16(size_t b) { return (b + 15) / 16 * 16; }

TripLds trip_lds(int nr, int lmax, int wg) {
    const int nlm = (lmax + 1) * (lmax + 1), rows = nlm + 1, nrp = nr | 1;
    TripLds o;
    size_t b = 0;
    o.e2 = (int)b; b += trip_al16((size_t)(nr + 1) * 8);
    o.tab = (int)b; b += trip_al16((size_t)FB_TRIP_TAB * 8);
    o.hi = (int)b; b += trip_al16((size_t)rows * nrp * 8);
    o.lo = (int)b; b += trip_al16((size_t)rows * nrp * 8);
    o.yt = (int)b; b += trip_al16((size_t)std::max(rows * FB_TRIP_YS, nlm * nr) * 8);
    o.ss = (int)b; b += trip_al16((size_t)FB_TRIP_MAX_NR * 8);
    o.sx = (int)b; b += (size_t)FB_TRIP_STAGE(wg) * 8;
    o.sy = (int)b; b += (size_t)FB_TRIP_STAGE(wg) * 8;
    o.sz = (int)b; b += (size_t)FB_TRIP_STAGE(wg) * 8;
    o.sw = (int)b; b += (size_t)FB_TRIP_STAGE(wg) * 8;
    o.sb = (int)b; b += (size_t)FB_TRIP_STAGE(wg) * 4;
    o.cnt = (int)b; b += (size_t)FB_TRIP_MAX_NR * 4;
    o.pairb = (int)b; b += trip_al16((size_t)(nr * (nr + 1) / 2) * 2);
    o.wtot = (int)b; b += trip_al16((size_t)FB_TRIP_MAX_NW * 4);
    o.probe = (int)b; b += (size_t)FB_TRIP_MAX_PROBE * 4;
    o.total = (int)b;
    return o;
}

// sw[slot] = w[perm[slot]]: the weights in the order of the permuted positions
__global__ __launch_bounds__(256) void k_trip_gather(const double* w, const unsigned* perm, unsigned long long n, double* sw) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256)
        sw[q] = w[perm[q]];
}

// the pair (b1 <= b2) number pi of the nr (nr + 1) / 2 pairs in the order (0, 0), (0, 1), ... (0, nr - 1), (1, 1), ...
__host__ __device__ __forceinline__ void trip_pair(int pi, int nr, int& b1, int& b2) {
    b1 = 0;
    for (int k = 0; k < FB_TRIP_MAX_NR; ++k) {
        if (pi < nr - b1) break;
        pi -= nr - b1;
        ++b1;
    }
    b2 = b1 + pi;
}

// One workgroup per primary in sorted order, grid-stride over the primaries.  The neighbour cells are walked as in
// k_centre_sweep of fb_profiles.hip: thread t takes slots q0 + t, q0 + t + WG, ... of a range, the primary skips its own
// slot -- "other" is decided by index, not by position -- and a neighbour is in bin b iff e2[b] <= d^2 < e2[b + 1], b by
// bisection; a neighbour with d^2 < e2[0] (e2[0] > 0: a coincident one included) is in no bin and no direction of it is
// formed.  The neighbours in range are compacted, by ballot and prefix count, into a stage in LDS: the unit vector d / sqrt(d^2)
// component by component, the weight and the bin.  Whenever the stage holds a tile of 64, and at the end for what is left:
//   B. lane j of wave v evaluates, for neighbour j of the tile, the harmonics of the orders m = v, v + WG / 64, ... by the
//      recurrence of the header comment -- the wave number is uniform, so the control flow is -- and writes w_j Y_lm to row lm
//      of the tile of harmonics (the last wave: w_j^2 to the last row);
//   C. thread (row, part) adds the terms of its part of the tile to the row's bins of the accumulator table in two-word
//      fixed point: LDS integer adds, so any order gives the same words.
// Then the table is read out as doubles a_lm(b) -- and cleared for the next primary --, the probed primaries' a_lm are
// written, and thread-owned entries (l, b1 <= b2) are formed in fp64, m ascending:
//   w_i ((4 pi / (2 l + 1)) sum_m a_lm(b1) a_lm(b2) - [b1 = b2] S(b1)),
// and added in two-word fixed point to the workgroup's own partial sums in global memory (plain read-modify-write of words
// only this thread touches).  Every loop is bounded by a cell's occupancy or a constant; nothing waits on data.
template <int WG>
__global__ __launch_bounds__(WG) void k_trip_sweep(TripArgs a, const double* tabg, const unsigned* start, const double* spos,
                                                           const double* sw, const unsigned* perm, const double* e2g,
                                                           const unsigned* probeg, unsigned long long* partial,
                                                           unsigned long long* pairs_out, double* alm_out) {
    constexpr int NW = WG / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* e2 = reinterpret_cast<double*>(smem + a.o.e2);
    double* tab = reinterpret_cast<double*>(smem + a.o.tab);
    unsigned long long* thi = reinterpret_cast<unsigned long long*>(smem + a.o.hi);
    unsigned long long* tlo = reinterpret_cast<unsigned long long*>(smem + a.o.lo);
    double* yt = reinterpret_cast<double*>(smem + a.o.yt);             // the tile of harmonics; then the a_lm as doubles
    double* sS = reinterpret_cast<double*>(smem + a.o.ss);
    double* stx = reinterpret_cast<double*>(smem + a.o.sx);
    double* sty = reinterpret_cast<double*>(smem + a.o.sy);
    double* stz = reinterpret_cast<double*>(smem + a.o.sz);
    double* stw = reinterpret_cast<double*>(smem + a.o.sw);
    int* stb = reinterpret_cast<int*>(smem + a.o.sb);
    unsigned* cnt = reinterpret_cast<unsigned*>(smem + a.o.cnt);
    unsigned short* pairb = reinterpret_cast<unsigned short*>(smem + a.o.pairb);
    unsigned* wtot = reinterpret_cast<unsigned*>(smem + a.o.wtot);
    unsigned* sprobe = reinterpret_cast<unsigned*>(smem + a.o.probe);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nr = a.nr, lmax = a.lmax, nlm = a.nlm, rows = a.rows, nrp = a.nrp;
    const FofGeom& g = a.g;
    for (int i = t; i <= nr; i += WG) e2[i] = e2g[i];
    for (int i = t; i < FB_TRIP_TAB; i += WG) tab[i] = tabg[i];
    for (int i = t; i < rows * nrp; i += WG) { thi[i] = 0ull; tlo[i] = 0ull; }
    for (int i = t; i < FB_TRIP_MAX_NR; i += WG) cnt[i] = 0u;
    for (int i = t; i < a.npair; i += WG) {
        int b1, b2;
        trip_pair(i, nr, b1, b2);
        pairb[i] = (unsigned short)((b1 << 8) | b2);
    }
    for (int i = t; i < a.nprobe; i += WG) sprobe[i] = probeg[i];
    __syncthreads();
    const double e2lo = e2[0], e2hi = e2[nr], sq2 = tab[FB_TRIP_TAB_SQ2];
    unsigned long long mypairs = 0ull;

    // one tile: the staged neighbours tb .. tb + tc - 1, tc <= 64 (the same in every thread)
    auto tile = [&](int tb, int tc) {
        {
            const bool v = lane < tc;
            const double x = v ? stx[tb + lane] : 0.0, y = v ? sty[tb + lane] : 0.0, z = v ? stz[tb + lane] : 1.0,
                         wj = v ? stw[tb + lane] : 0.0;
            double c = 1.0, s = 0.0;
            int mm = 0;
            for (int m = wave; m <= lmax; m += NW) {
                for (; mm < m; ++mm) {
                    const double cn = x * c - y * s, sn = x * s + y * c;
                    c = cn; s = sn;
                }
                double qm2 = 0.0, qm1 = tab[FB_TRIP_TAB_A + m];
                for (int l = m; l <= lmax; ++l) {
                    double q = qm1;
                    if (l == m + 1) q = (tab[FB_TRIP_TAB_G + m] * z) * qm1;
                    else if (l > m + 1) q = tab[FB_TRIP_TAB_AL + l * FB_TRIP_NT + m] * (z * qm1 - tab[FB_TRIP_TAB_BE + l * FB_TRIP_NT + m] * qm2);
                    if (l > m) { qm2 = qm1; qm1 = q; }
                    const int l0 = l * l + l;
                    if (m == 0) yt[l0 * FB_TRIP_YS + lane] = wj * q;
                    else {
                        const double sq = sq2 * q;
                        yt[(l0 + m) * FB_TRIP_YS + lane] = wj * (sq * c);
                        yt[(l0 - m) * FB_TRIP_YS + lane] = wj * (sq * s);
                    }
                }
            }
            if (wave == NW - 1) yt[nlm * FB_TRIP_YS + lane] = wj * wj;
        }
        __syncthreads();
        if (t < rows * a.parts) {
            const int row = t % rows, part = t / rows;
            const int j0 = part * a.per, j1 = min(tc, j0 + a.per);
            const int F = row == nlm ? a.Fs : a.Fa;
            for (int j = j0; j < j1; j += 4) {                        // four loads in flight before the first add
                int b[4];
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int jj = min(j + u, j1 - 1);
                    b[u] = stb[tb + jj];
                    v[u] = yt[row * FB_TRIP_YS + jj];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j + u >= j1) break;
                    unsigned long long hi, lo;
                    fx_split(ldexp(v[u], F), hi, lo);
                    atomicAdd(&thi[row * nrp + b[u]], hi);
                    atomicAdd(&tlo[row * nrp + b[u]], lo);
                }
            }
        }
        __syncthreads();                                              // the stage and the tile of harmonics are free again
    };

    for (unsigned long long p = blockIdx.x; p < a.n; p += gridDim.x) {
        const double w0 = spos[3 * p], w1 = spos[3 * p + 1], w2 = spos[3 * p + 2];     // wrapped by k_fof_scatter
        const double wi = sw ? sw[p] : 1.0;
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
        int nst = 0;                                                  // staged neighbours: the same in every thread
        for (int o0 = g.nc[0] < 3 ? 0 : -1; o0 <= 1; ++o0) {
            const int m0 = (c0 + o0 + g.nc[0]) % g.nc[0];
            for (int o1 = g.nc[1] < 3 ? 0 : -1; o1 <= 1; ++o1) {
                const int m1 = (c1 + o1 + g.nc[1]) % g.nc[1];
                const unsigned base = ((unsigned)m0 * (unsigned)g.nc[1] + (unsigned)m1) * (unsigned)g.nc[2];
                for (int r = 0; r < nrange; ++r) {
                    const unsigned q1 = start[base + (unsigned)zhi[r]];
                    for (unsigned qb = start[base + (unsigned)zlo[r]]; qb < q1; qb += WG) {
                        const unsigned q = qb + (unsigned)t;
                        bool in = false;
                        double dx = 0.0, dy = 0.0, dz = 0.0, d2 = 0.0;
                        if (q < q1 && (unsigned long long)q != p) {
                            dx = fof_min_image(spos[3ull * q] - w0, g.L[0]);
                            dy = fof_min_image(spos[3ull * q + 1] - w1, g.L[1]);
                            dz = fof_min_image(spos[3ull * q + 2] - w2, g.L[2]);
                            d2 = (dx * dx + dy * dy) + dz * dz;
                            in = d2 >= e2lo && d2 < e2hi;
                        }
                        const unsigned long long mask = __ballot(in);
                        if (lane == 0) wtot[wave] = (unsigned)__popcll(mask);
                        __syncthreads();
                        int before = 0, total = 0;                 // in range in the waves before this one, and in all
                        for (int k = 0; k < NW; ++k) {
                            const int ck = (int)wtot[k];
                            if (k < wave) before += ck;
                            total += ck;
                        }
                        if (in) {
                            int lo = 0, hi = nr - 1;                  // the largest b with e2[b] <= d2
                            for (int s = 0; s < a.rsteps; ++s) {
                                const int mid = (lo + hi + 1) >> 1;
                                if (e2[mid] <= d2) lo = mid; else hi = mid - 1;
                            }
                            const int off = nst + before + __popcll(mask & ((1ull << lane) - 1ull));
                            const double rr = sqrt(d2);
                            stx[off] = dx / rr; sty[off] = dy / rr; stz[off] = dz / rr;
                            stw[off] = sw ? sw[q] : 1.0;
                            stb[off] = lo;
                            atomicAdd(&cnt[lo], 1u);
                        }
                        nst += total;
                        __syncthreads();                              // the stage is written, wtot has been read
                        while (nst >= FB_TRIP_TILE) {
                            nst -= FB_TRIP_TILE;
                            tile(nst, FB_TRIP_TILE);
                        }
                    }
                }
            }
        }
        if (nst > 0) tile(0, nst);
        // the table as doubles, cleared for the next primary
        for (int i = t; i < nlm * nr; i += WG) {
            const int lm = i / nr, b = i - lm * nr, k = lm * nrp + b;
            yt[i] = fx_join(thi[k], tlo[k], a.Fa);
            thi[k] = 0ull; tlo[k] = 0ull;
        }
        if (t < nr) {
            const int k = nlm * nrp + t;
            sS[t] = fx_join(thi[k], tlo[k], a.Fs);
            thi[k] = 0ull; tlo[k] = 0ull;
            mypairs += cnt[t];
            cnt[t] = 0u;
        }
        __syncthreads();
        if (a.nprobe) {
            const unsigned orig = perm[p];
            for (int k = 0; k < a.nprobe; ++k) {
                if (sprobe[k] != orig) continue;
                for (int i = t; i < nlm * nr; i += WG) alm_out[(size_t)k * (size_t)(nlm * nr) + i] = yt[i];
            }
        }
        for (int e = t; e < a.nent; e += WG) {
            const int l = e / a.npair, pi = e - l * a.npair;
            const int b1 = pairb[pi] >> 8, b2 = pairb[pi] & 255;
            double sum = 0.0;
            for (int lm = l * l; lm <= l * l + 2 * l; ++lm) sum += yt[lm * nr + b1] * yt[lm * nr + b2];
            double val = tab[FB_TRIP_TAB_FL + l] * sum;
            if (b1 == b2) val = val - sS[b1];
            val = wi * val;
            unsigned long long hi, lo;
            fx_split(ldexp(val, a.Fm), hi, lo);
            unsigned long long* dst = partial + 2ull * ((unsigned long long)blockIdx.x * (unsigned long long)a.nent + (unsigned long long)e);
            dst[0] += hi;
            dst[1] += lo;
        }
        __syncthreads();                                              // the a_lm have been read before the next tile of harmonics
    }
    if (t < nr && mypairs) atomicAdd(&pairs_out[t], mypairs);
}

// M[l][b1][b2] = M[l][b2][b1] = the sum of the workgroups' partial words, joined: integer adds in a fixed order
__global__ __launch_bounds__(256) void k_trip_finish(const unsigned long long* partial, int nwg, int nent, int npair, int nr, int Fm,
                                                     double* M_out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nent) return;
    unsigned long long hi = 0ull, lo = 0ull;
    for (int w = 0; w < nwg; ++w) {
        hi += partial[2ull * ((unsigned long long)w * (unsigned long long)nent + (unsigned long long)e)];
        lo += partial[2ull * ((unsigned long long)w * (unsigned long long)nent + (unsigned long long)e) + 1];
    }
    const int l = e / npair;
    int b1, b2;
    trip_pair(e - l * npair, nr, b1, b2);
    const double v = fx_join(hi, lo, Fm);
    M_out[((size_t)l * nr + b1) * nr + b2] = v;
    M_out[((size_t)l * nr + b2) * nr + b1] = v;
}

// the work buffer: small | e2 f64[33] | tab f64[276] | probe u32[64] | spos f64[3 n] | sw f64[n] (weighted) | start u32[ncells + 1]
// | cursor u32[ncells] | csum u32[chunks] | cellid u32[n] | perm u32[n] | partial u64[512][nent][2]
struct TripWork { size_t e2, tab, probe, spos, sw, start, cursor, csum, cellid, perm, partial, total; };
TripWork trip_layout(unsigned long long n, unsigned long long ncells, int nr, int lmax, bool weighted) {
    TripWork w;
    size_t o = FB_TRIP_SMALL;
    w.e2 = o; o += align16((size_t)(FB_TRIP_MAX_NR + 1) * 8);
    w.tab = o; o += align16((size_t)FB_TRIP_TAB * 8);
    w.probe = o; o += align16((size_t)FB_TRIP_MAX_PROBE * 4);
    w.spos = o; o += align16((size_t)n * 24);
    w.sw = o; o += weighted ? align16((size_t)n * 8) : 0;
    w.start = o; o += align16((size_t)(ncells + 1) * 4);
    w.cursor = o; o += align16((size_t)ncells * 4);
    w.csum = o; o += align16((size_t)scan_chunks(ncells) * 4);
    w.cellid = o; o += align16((size_t)n * 4);
    w.perm = o; o += align16((size_t)n * 4);
    w.partial = o; o += (size_t)FB_TRIP_MAX_WG * (size_t)((lmax + 1) * (nr * (nr + 1) / 2)) * 16;
    w.total = o;
    return w;
}

// the constants of the recurrence, each formed in fp64 as the numpy statement forms it
void trip_table(double* tab) {
    for (int i = 0; i < FB_TRIP_TAB; ++i) tab[i] = 0.0;
    tab[FB_TRIP_TAB_A] = std::sqrt(1.0 / (4.0 * M_PI));
    for (int m = 1; m <= FB_TRIP_MAX_L; ++m) tab[FB_TRIP_TAB_A + m] = tab[FB_TRIP_TAB_A + m - 1] * std::sqrt((2.0 * m + 1.0) / (2.0 * m));
    for (int m = 0; m <= FB_TRIP_MAX_L; ++m) tab[FB_TRIP_TAB_G + m] = std::sqrt(2.0 * m + 3.0);
    for (int l = 2; l <= FB_TRIP_MAX_L; ++l)
        for (int m = 0; m <= l - 2; ++m) {
            const double dl = (double)l, dm = (double)m, d1 = dl - 1.0;
            tab[FB_TRIP_TAB_AL + l * FB_TRIP_NT + m] = std::sqrt((4.0 * dl * dl - 1.0) / (dl * dl - dm * dm));
            tab[FB_TRIP_TAB_BE + l * FB_TRIP_NT + m] = std::sqrt((d1 * d1 - dm * dm) / (4.0 * d1 * d1 - 1.0));
        }
    for (int l = 0; l <= FB_TRIP_MAX_L; ++l) tab[FB_TRIP_TAB_FL + l] = (4.0 * M_PI) / (2.0 * l + 1.0);
    tab[FB_TRIP_TAB_SQ2] = std::sqrt(2.0);
}

int trip_bits(double bound) {
    int e = 0;
    if (bound > 0.0) (void)frexp(bound, &e);
    return 93 - e;
}

}  // namespace

extern "C" {

int64_t fb_triplet_work_bytes(int64_t n, int64_t ncells, int nr, int lmax, int weighted) {
    if (n < 0 || n > 2147483646ll || ncells < 1 || ncells > (1ll << 31) || nr < 1 || nr > FB_TRIP_MAX_NR || lmax < 0 || lmax > FB_TRIP_MAX_L)
        return -1;
    return (int64_t)trip_layout((unsigned long long)n, (unsigned long long)ncells, nr, lmax, weighted != 0).total;
}

int fb_triplet_multipoles(fb_plan* p, const double* pos, const double* w, int64_t n, const int* ncell, const double* edges2, int nr,
                          int lmax, void* work, int64_t work_bytes, double* M_out, uint64_t* pairs_out, const int32_t* probe_idx,
                          int nprobe, double* alm_out, int* bad, double* stage_ms, void* stream) {
    FB_REQUIRE(p && ncell && edges2 && work && M_out && pairs_out && bad, "null pointer");
    FB_REQUIRE(n >= 0 && n <= 2147483646ll, "triplets: 0 <= n <= 2^31 - 2");
    FB_REQUIRE(nr >= 1 && nr <= FB_TRIP_MAX_NR, "triplets: 1 <= nr <= 32");
    FB_REQUIRE(lmax >= 0 && lmax <= FB_TRIP_MAX_L, "triplets: 0 <= lmax <= 10");
    FB_REQUIRE(edges2[0] > 0.0, "triplets: edges[0] > 0");
    for (int b = 0; b < nr; ++b) FB_REQUIRE(edges2[b] < edges2[b + 1], "triplets: strictly ascending edges");       // NaN fails
    unsigned long long ncells = 1;
    for (int a = 0; a < 3; ++a) {
        FB_REQUIRE(ncell[a] >= 2, "triplets: at least 2 cells per axis");
        ncells *= (unsigned long long)ncell[a];
        FB_REQUIRE(ncells <= (1ull << 31), "triplets: at most 2^31 cells");
        const double side = p->L[a] / (double)ncell[a];
        FB_REQUIRE(edges2[nr] < 0.25 * p->L[a] * p->L[a] && side * side >= edges2[nr],
                   "triplets: the last edge must stay below L / 2 and within the side of the cells");
    }
    FB_REQUIRE(nprobe >= 0 && nprobe <= FB_TRIP_MAX_PROBE, "triplets: at most 64 probed primaries");
    FB_REQUIRE(nprobe == 0 || (probe_idx && alm_out), "null pointer");
    for (int k = 0; k < nprobe; ++k) FB_REQUIRE(probe_idx[k] >= 0 && (int64_t)probe_idx[k] < n, "triplets: a probed index outside 0 .. n - 1");
    const bool weighted = w != nullptr;
    const TripWork wl = trip_layout((unsigned long long)n, ncells, nr, lmax, weighted);
    FB_REQUIRE(work_bytes >= (int64_t)wl.total, "triplets: work buffer smaller than fb_triplet_work_bytes");
    FB_REQUIRE(n == 0 || pos, "null pointer");
    const int wg = (lmax + 1) * (lmax + 1) + 1 > 64 ? FB_TRIP_WG_LARGE : FB_TRIP_WG_SMALL;
    const TripLds lds = trip_lds(nr, lmax, wg);
    FB_REQUIRE(lds.total <= FB_TRIP_LDS_MAX, "triplets: (lmax + 1)^2 x nr does not fit the LDS");
    *bad = 0;
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.0;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const int nlm = (lmax + 1) * (lmax + 1), npair = nr * (nr + 1) / 2, nent = (lmax + 1) * npair;
    FB_HIP(hipMemsetAsync(M_out, 0, (size_t)(lmax + 1) * nr * nr * 8, s));
    FB_HIP(hipMemsetAsync(pairs_out, 0, (size_t)nr * 8, s));
    if (nprobe) FB_HIP(hipMemsetAsync(alm_out, 0, (size_t)nprobe * nlm * nr * 8, s));
    if (n == 0) {
        FB_HIP(hipStreamSynchronize(s));
        return FB_OK;
    }
    char* wb = (char*)work;
    TripSmall* sm = (TripSmall*)wb;
    double *e2d = (double*)(wb + wl.e2), *tabd = (double*)(wb + wl.tab), *spos = (double*)(wb + wl.spos),
           *swd = weighted ? (double*)(wb + wl.sw) : nullptr;
    unsigned *probed = (unsigned*)(wb + wl.probe), *start = (unsigned*)(wb + wl.start), *cursor = (unsigned*)(wb + wl.cursor),
             *csum = (unsigned*)(wb + wl.csum), *cellid = (unsigned*)(wb + wl.cellid), *perm = (unsigned*)(wb + wl.perm);
    unsigned long long* partial = (unsigned long long*)(wb + wl.partial);
    const FofGeom g = geom_of(p, ncell);
    const unsigned long long un = (unsigned long long)n;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (stage_ms) for (int q = 0; q < 4; ++q) FB_HIP(hipEventCreate(&ev[q]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int q = 0; q < 4; ++q) if (e[q]) (void)hipEventDestroy(e[q]); } } evg{ev};
    if (stage_ms) FB_HIP(hipEventRecord(ev[0], s));
    FB_HIP(hipMemsetAsync(sm, 0, FB_TRIP_SMALL, s));
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_bin, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, cellid, cursor, &sm->err);
    FB_LAUNCH_CHECK("k_fof_bin");
    if (weighted) {
        hipLaunchKernelGGL(k_fof_vmax, dim3(grid_for(un, p)), dim3(256), 0, s, w, un, &sm->wmax_bits, &sm->err);
        FB_LAUNCH_CHECK("k_fof_vmax");
    }
    TripSmall h;
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    if (h.err & FB_FOF_ERR_POS) { *bad = 1; return FB_OK; }
    // every |sum| stays below 2^e.  |Y_lm| < 2, so |a_lm(b)| < 2 n wmax; S(b) <= n wmax^2; and, by the addition theorem,
    // |4 pi / (2 l + 1) sum_m a_lm(b1) a_lm(b2)| <= A(b1) A(b2) <= (n wmax)^2, so |M| <= 2 (n wmax)^3: twice that for rounding
    double wmax = 1.0;
    if (weighted) memcpy(&wmax, &h.wmax_bits, sizeof(wmax));
    const double nw = (double)n * wmax, bound_m = 4.0 * nw * nw * nw;
    if ((h.err & FB_FOF_ERR_VEL) || !std::isfinite(bound_m)) { *bad = 4; return FB_OK; }
    FB_TRY(exscan(ScanPlain{cursor}, ncells, csum, start, s));       // start[ncells] = n
    FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
    hipLaunchKernelGGL(k_fof_scatter, dim3(grid_for(un, p)), dim3(256), 0, s, pos, un, g, (const unsigned*)cellid, (const unsigned*)start,
                       cursor, perm, spos, (unsigned*)nullptr);
    FB_LAUNCH_CHECK("k_fof_scatter");
    if (weighted) {
        hipLaunchKernelGGL(k_trip_gather, dim3(grid_for(un, p)), dim3(256), 0, s, w, (const unsigned*)perm, un, swd);
        FB_LAUNCH_CHECK("k_trip_gather");
    }
    double tabh[FB_TRIP_TAB];
    trip_table(tabh);
    unsigned probeh[FB_TRIP_MAX_PROBE] = {0};
    for (int k = 0; k < nprobe; ++k) probeh[k] = (unsigned)probe_idx[k];
    FB_HIP(hipMemcpyAsync(e2d, edges2, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, s));
    FB_HIP(hipMemcpyAsync(tabd, tabh, sizeof(tabh), hipMemcpyHostToDevice, s));
    FB_HIP(hipMemcpyAsync(probed, probeh, sizeof(probeh), hipMemcpyHostToDevice, s));
    const int nwg = (int)std::min<unsigned long long>(un, std::min<unsigned long long>(FB_TRIP_MAX_WG, 2ull * (unsigned long long)p->num_cu));
    FB_HIP(hipMemsetAsync(partial, 0, (size_t)nwg * nent * 16, s));
    TripArgs a;
    a.g = g; a.n = un;
    a.nr = nr; a.lmax = lmax; a.nlm = nlm; a.rows = nlm + 1; a.nrp = nr | 1;
    a.rsteps = 0;
    while ((1 << a.rsteps) < nr) ++a.rsteps;
    a.parts = std::min(FB_TRIP_TILE, wg / a.rows);
    a.per = (FB_TRIP_TILE + a.parts - 1) / a.parts;
    a.npair = npair; a.nent = nent; a.nprobe = nprobe;
    a.Fa = trip_bits(2.0 * nw); a.Fs = trip_bits((double)n * wmax * wmax); a.Fm = trip_bits(bound_m);
    a.o = lds;
    if (stage_ms) FB_HIP(hipEventRecord(ev[1], s));
    const void* fn = wg == FB_TRIP_WG_LARGE ? reinterpret_cast<const void*>(k_trip_sweep<FB_TRIP_WG_LARGE>)
                                            : reinterpret_cast<const void*>(k_trip_sweep<FB_TRIP_WG_SMALL>);
    if (lds.total > 65536) FB_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds.total));
#define FB_TRIP_LAUNCH(W) hipLaunchKernelGGL(k_trip_sweep<W>, dim3(nwg), dim3(W), (size_t)lds.total, s, a, (const double*)tabd, \
                       (const unsigned*)start, (const double*)spos, (const double*)swd, (const unsigned*)perm, (const double*)e2d, \
                       (const unsigned*)probed, partial, (unsigned long long*)pairs_out, alm_out)
    if (wg == FB_TRIP_WG_LARGE) FB_TRIP_LAUNCH(FB_TRIP_WG_LARGE); else FB_TRIP_LAUNCH(FB_TRIP_WG_SMALL);
#undef FB_TRIP_LAUNCH
    FB_LAUNCH_CHECK("k_trip_sweep");
    if (stage_ms) FB_HIP(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(k_trip_finish, dim3((nent + 255) / 256), dim3(256), 0, s, (const unsigned long long*)partial, nwg, nent, npair, nr,
                       a.Fm, M_out);
    FB_LAUNCH_CHECK("k_trip_finish");
    if (stage_ms) FB_HIP(hipEventRecord(ev[3], s));
    FB_HIP(hipStreamSynchronize(s));                                  // the host tables live on this stack
    if (stage_ms) {
        for (int q = 0; q < 3; ++q) {
            float ms = 0.f;
            FB_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            stage_ms[q] = (double)ms;
        }
    }
    return FB_OK;
}

}  // extern "C"
