// Pair counts of periodic catalogues in separation bins (nbodykit's SimulationBox2PCF): both catalogues
// are binned into one grid of cells (fb_cells.h, shared with fb_fof.hip), then every pair of a home particle and a particle of
// a distinct neighbour cell is tested once and counted into an integer histogram.  Particle data are fp64 whatever the plan's
// precision; the plan gives the box and the device.  See include/fastbox_hip.h for the entry points.
//
// No contraction anywhere in this file: the minimum-image differences, d^2 = (dx dx + dy dy) + dz dz and the products of the
// mu test must be the doubles of the numpy statement (tests/pairs_numpy.py), so that a pair on an edge falls on the device
// into the bin it falls into there.  No square root is taken: every comparison is between squares.
#pragma clang fp contract(off)
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_cells.h"
#include <algorithm>
#include <cmath>

#define FB_PAIR_SMALL 256                // bytes at the head of the work buffer: the words of PairSmall
#define FB_PAIR_WG 256                   // threads per workgroup of the sweep: 4 waves share one home tile and one histogram
#define FB_PAIR_NTILE 256                // neighbour particles per LDS tile: 64 per wave
#define FB_PAIR_MAX_NR 256
#define FB_PAIR_MAX_BINS 4096            // words of the LDS histogram: bins x interleaved copies
#define FB_PAIR_FLUSH (1u << 31)         // pair tests of one workgroup between two flushes of its histogram (fb_debug_pair_flush)

namespace {

struct PairSmall { unsigned err, items, pad[2]; };

struct PairBins {
    int mode;                            // 0: r; 1: (r, mu); 2: (r_p, pi)
    int nr, nsub;                        // radial bins, sub bins (1 in mode 0)
    int rsteps, ssteps;                  // bounds of the two bisections: ceil(log2(nr)), ceil(log2(nsub))
    int copies_log2;                     // interleaved copies of the LDS histogram
    unsigned flush;                      // the workgroup flushes once it has tested this many pairs: at most 2^31
    double sub_a;                        // mode 1: Nmu^2; else 1
    double sub_max2;                     // mode 2: pimax^2
};

// one pair: home particle (hx, hy, hz) in slot hs, neighbour (nx, ny, nz) in slot ns; `same`: both in the home cell of auto-counts
__device__ __forceinline__ void pair_add(const FofGeom& g, const PairBins& pb, const double* e2, double e2lo, double e2hi, unsigned* hist,
                                         unsigned copy, int self_mode, bool same, double hx, double hy, double hz, unsigned hs,
                                         double nx, double ny, double nz, unsigned ns) {
    if (same && (self_mode == 1 ? hs >= ns : hs == ns)) return;
    const double dx = fof_min_image(hx - nx, g.L[0]), dy = fof_min_image(hy - ny, g.L[1]), dz = fof_min_image(hz - nz, g.L[2]);
    const double rp2 = dx * dx + dy * dy, zz = dz * dz;
    const double d2 = rp2 + zz;
    const double v = pb.mode == 2 ? rp2 : d2;
    if (!(v >= e2lo && v < e2hi)) return;
    if (pb.mode == 2 && zz >= pb.sub_max2) return;
    int lo = 0, hi = pb.nr - 1;                                       // the largest b with e2[b] <= v
    for (int s = 0; s < pb.rsteps; ++s) {
        const int mid = (lo + hi + 1) >> 1;
        if (e2[mid] <= v) lo = mid; else hi = mid - 1;
    }
    int sl = 0, sh = pb.nsub - 1;                                     // the largest j with zz A >= j j B (j = 0: always)
    if (pb.mode) {
        const double lhs = zz * pb.sub_a, B = pb.mode == 1 ? d2 : 1.0;
        for (int s = 0; s < pb.ssteps; ++s) {
            const int mid = (sl + sh + 1) >> 1;
            if (lhs >= (double)(mid * mid) * B) sl = mid; else sh = mid - 1;
        }
    }
    atomicAdd(&hist[((unsigned)(lo * pb.nsub + sl) << pb.copies_log2) + copy], 1u);
}

// the workgroup's histogram into the global one: the copies of a bin are summed first (64-bit: up to 64 counters below 2^32),
// so that a workgroup sends one atomic per bin that is not empty -- the global words are few and every workgroup adds to them
__device__ __forceinline__ void pair_flush(unsigned* hist, unsigned long long* out, int nbins, int copies_log2, unsigned long long mult,
                                           bool zero) {
    const int nc = 1 << copies_log2;
    for (int b = threadIdx.x; b < nbins; b += FB_PAIR_WG) {
        unsigned long long sum = 0;
        for (int q = 0; q < nc; ++q) {
            const int w = (b << copies_log2) + ((q + b) & (nc - 1));   // start at copy b: the threads of a wave on different banks
            sum += hist[w];
            if (zero) hist[w] = 0u;
        }
        if (sum) atomicAdd(&out[b], mult * sum);
    }
}

// One workgroup of four waves per (home cell, home tile of 64): lane l of every wave keeps home particle l of the tile in
// registers; the particles of the distinct neighbour cells go through LDS in tiles of 256, and wave w walks entries
// 64 w ... 64 w + 63 of the tile -- all lanes of a wave read one LDS address, a broadcast.  Where the home tile holds fewer
// particles than a wave would walk (a sparse catalogue against a dense one: one or two halos per cell against a thousand
// particles) the roles are exchanged for that tile: thread t keeps neighbour t and walks the home particles, which are in LDS
// too, so that all 256 threads have a pair instead of one or two lanes of each wave.  A pair is decided by its own
// minimum-image differences.  The radial bin is found by bisection over e2 = edges^2 in LDS, the mu / pi bin by bisection
// over j of the monotone test  dz dz A >= j j B  (A = Nmu^2, B = d^2; or A = B = 1), and the count goes to copy (lane mod
// copies) of the workgroup's LDS histogram: neighbouring lanes that hit one bin hit different banks, not one word.
//
// self_mode 0 (cross-counts): every (home, neighbour) pair.  1 (auto, half shell: 3 or more cells on every axis): the cell
// itself with each pair once by slot order, and the 13 neighbours of the upper half shell, each adjacent pair of cells once;
// the flush doubles.  2 (auto, fewer than 3 cells on some axis): all distinct neighbour cells, inside the home cell every
// ordered pair of different slots; no doubling.  With 2 cells on an axis the offsets -1 and +1 name one cell: it is visited
// once, by offset +1.
//
// The LDS counters are 32-bit: a workgroup flushes to the global 64-bit histogram before the pairs it has tested since its
// last flush could pass 2^31 + 2^14 (pb.flush <= 2^31; one tile adds at most 64 x 256), so no counter wraps.  items NULL: work item w is tile 0
// of cell w; else the (cell, tile) pair items[2 w], items[2 w + 1].  Every loop is bounded by a cell's occupancy or a constant.
__global__ __launch_bounds__(FB_PAIR_WG) void k_pair_sweep(FofGeom g, const unsigned* hstart, const double* hpos, const unsigned* nstart,
                                                          const double* npos, const double* e2g, PairBins pb, int self_mode,
                                                          const unsigned* items, unsigned long long total,
                                                          unsigned long long* out) {
    __shared__ double e2[FB_PAIR_MAX_NR + 1];
    __shared__ double tx[FB_PAIR_NTILE], ty[FB_PAIR_NTILE], tz[FB_PAIR_NTILE];
    __shared__ double hsx[FB_FOF_TILE], hsy[FB_FOF_TILE], hsz[FB_FOF_TILE];
    __shared__ unsigned hist[FB_PAIR_MAX_BINS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nbins = pb.nr * pb.nsub, nwords = nbins << pb.copies_log2;
    const unsigned copy = (unsigned)lane & ((1u << pb.copies_log2) - 1u);
    const unsigned long long mult = self_mode == 1 ? 2ull : 1ull;
    for (int i = t; i <= pb.nr; i += FB_PAIR_WG) e2[i] = e2g[i];
    for (int i = t; i < nwords; i += FB_PAIR_WG) hist[i] = 0u;
    __syncthreads();
    const double e2lo = e2[0], e2hi = e2[pb.nr];
    unsigned since = 0;                                              // pair tests since the last flush: the same in every thread
    for (unsigned long long w = blockIdx.x; w < total; w += gridDim.x) {
        const unsigned c = items ? items[2 * w] : (unsigned)w, k = items ? items[2 * w + 1] : 0u;
        const unsigned b0 = hstart[c], b1 = hstart[c + 1];
        if (b1 - b0 <= k * FB_FOF_TILE) continue;                     // no home particle: the whole workgroup skips it
        const unsigned h0 = b0 + k * FB_FOF_TILE;
        const int nh = (int)min(b1 - h0, (unsigned)FB_FOF_TILE);
        const bool live = lane < nh;
        const unsigned hs = h0 + (unsigned)lane;
        const double hx = live ? hpos[3ull * hs] : 0.0, hy = live ? hpos[3ull * hs + 1] : 0.0, hz = live ? hpos[3ull * hs + 2] : 0.0;
        __syncthreads();                                              // the last tile of the previous item has been walked
        if (wave == 0 && live) { hsx[lane] = hx; hsy[lane] = hy; hsz[lane] = hz; }      // read after the barriers of the first tile
        const int c2 = (int)(c % (unsigned)g.nc[2]), c1 = (int)((c / (unsigned)g.nc[2]) % (unsigned)g.nc[1]),
                  c0 = (int)(c / ((unsigned)g.nc[2] * (unsigned)g.nc[1]));
        for (int o = self_mode == 1 ? 13 : 0; o < 27; ++o) {
            const int o0 = o / 9 - 1, o1 = (o / 3) % 3 - 1, o2 = o % 3 - 1;
            if ((o0 < 0 && g.nc[0] < 3) || (o1 < 0 && g.nc[1] < 3) || (o2 < 0 && g.nc[2] < 3)) continue;   // -1 is +1 there
            const int m0 = (c0 + o0 + g.nc[0]) % g.nc[0], m1 = (c1 + o1 + g.nc[1]) % g.nc[1], m2 = (c2 + o2 + g.nc[2]) % g.nc[2];
            const unsigned m = ((unsigned)m0 * (unsigned)g.nc[1] + (unsigned)m1) * (unsigned)g.nc[2] + (unsigned)m2;
            const bool same = self_mode != 0 && m == c;
            const unsigned q1 = nstart[m + 1];
            for (unsigned q0 = nstart[m]; q0 < q1; q0 += FB_PAIR_NTILE) {
                const int nn = (int)min(q1 - q0, (unsigned)FB_PAIR_NTILE);
                __syncthreads();                                      // the previous tile has been walked
                if (since >= pb.flush) {
                    pair_flush(hist, out, nbins, pb.copies_log2, mult, true);
                    since = 0;
                    __syncthreads();
                }
                if (t < nn) { tx[t] = npos[3ull * (q0 + t)]; ty[t] = npos[3ull * (q0 + t) + 1]; tz[t] = npos[3ull * (q0 + t) + 2]; }
                since += (unsigned)(nh * nn);
                __syncthreads();
                if (nh < min(nn, 64)) {                              // few home particles: thread t takes neighbour t, walks them
                    if (t < nn) for (int i = 0; i < nh; ++i)
                        pair_add(g, pb, e2, e2lo, e2hi, hist, copy, self_mode, same, hsx[i], hsy[i], hsz[i], h0 + (unsigned)i, tx[t], ty[t],
                                 tz[t], q0 + (unsigned)t);
                } else if (live) {                                    // lane l keeps home particle l, wave w walks its quarter
                    const int j1 = min(nn, 64 * wave + 64);
                    for (int j = 64 * wave; j < j1; ++j)
                        pair_add(g, pb, e2, e2lo, e2hi, hist, copy, self_mode, same, hx, hy, hz, hs, tx[j], ty[j], tz[j], q0 + (unsigned)j);
                }
            }
        }
    }
    __syncthreads();
    pair_flush(hist, out, nbins, pb.copies_log2, mult, false);
}

unsigned g_pair_flush = FB_PAIR_FLUSH;   // fb_debug_pair_flush

int ceil_log2(int n) {
    int s = 0;
    while ((1 << s) < n) ++s;
    return s;
}

// per catalogue: spos f64[3 n] | start u32[ncells + 1] | cursor u32[ncells] | cellid u32[n]
struct PairCat { size_t spos, start, cursor, cellid; };
// the work buffer of fb_pair_count: small | e2 f64[257] | catalogue 1 | catalogue 2 (n2 > 0) | csum u32[chunks] |
// items u32[2 (n1 / TILE + 1)]
struct PairWork { size_t e2; PairCat cat[2]; size_t csum, items, total; };
PairWork pair_layout(unsigned long long n1, unsigned long long n2, unsigned long long ncells) {
    PairWork w;
    size_t o = FB_PAIR_SMALL;
    w.e2 = o; o += align16((size_t)(FB_PAIR_MAX_NR + 1) * 8);
    const unsigned long long n[2] = {n1, n2};
    for (int q = 0; q < 2; ++q) {
        w.cat[q].spos = o; o += align16((size_t)n[q] * 24);
        w.cat[q].start = o; o += align16((size_t)(ncells + 1) * 4);
        w.cat[q].cursor = o; o += align16((size_t)ncells * 4);
        w.cat[q].cellid = o; o += align16((size_t)n[q] * 4);
    }
    w.csum = o; o += align16((size_t)scan_chunks(ncells) * 4);
    w.items = o; o += align16((size_t)(n1 / FB_FOF_TILE + 1) * 8);
    w.total = o;
    return w;
}

}  // namespace

extern "C" {

int fb_debug_pair_flush(int64_t pairs) {
    FB_REQUIRE(pairs >= 0 && pairs <= (int64_t)FB_PAIR_FLUSH, "pair counts: a flush threshold of 1 .. 2^31 pair tests, or 0 for the default");
    g_pair_flush = pairs ? (unsigned)pairs : FB_PAIR_FLUSH;
    return FB_OK;
}

int64_t fb_pair_work_bytes(int64_t n1, int64_t n2, int64_t ncells) {
    if (n1 < 0 || n2 < 0 || ncells < 1) return -1;
    return (int64_t)pair_layout((unsigned long long)n1, (unsigned long long)n2, (unsigned long long)ncells).total;
}

int fb_pair_count(fb_plan* p, const double* pos1, int64_t n1, const double* pos2, int64_t n2, int mode, const double* edges2, int nr,
                  int nsub, double sub_max, const int* ncell, void* work, int64_t work_bytes, uint64_t* counts_out, int* bad,
                  double* stage_ms, void* stream) {
    FB_REQUIRE(p && edges2 && ncell && work && counts_out && bad, "null pointer");
    const bool autoc = pos2 == nullptr;
    if (autoc) n2 = 0;
    FB_REQUIRE(n1 >= 0 && n1 <= 2147483646ll && n2 >= 0 && n2 <= 2147483646ll, "pair counts: 0 <= n <= 2^31 - 2");
    FB_REQUIRE(mode >= 0 && mode <= 2, "pair counts: mode 0 (r), 1 (r, mu) or 2 (r_p, pi)");
    FB_REQUIRE(nr >= 1 && nr <= FB_PAIR_MAX_NR && nsub >= 1 && (mode != 0 || nsub == 1) && (int64_t)nr * nsub <= FB_PAIR_MAX_BINS,
               "pair counts: 1 <= nr <= 256 and nr x nsub <= 4096 bins (nsub = 1 in mode 0)");
    FB_REQUIRE(edges2[0] >= 0.0, "pair counts: edges[0] >= 0");
    for (int b = 0; b < nr; ++b) FB_REQUIRE(edges2[b] < edges2[b + 1], "pair counts: strictly ascending edges");   // NaN fails
    const double e2max = edges2[nr];
    // the reach along every axis: cells must be at least that long, and it must stay below half the box (one image only)
    double reach2[3] = {e2max, e2max, e2max};
    if (mode == 2) {
        FB_REQUIRE(sub_max > 0.0 && (double)nsub == sub_max, "pair counts: pimax a positive integer, one pi bin per Mpc");
        reach2[2] = sub_max * sub_max;
    }
    unsigned long long ncells = 1;
    for (int a = 0; a < 3; ++a) {
        FB_REQUIRE(reach2[a] < 0.25 * p->L[a] * p->L[a], "pair counts: the largest separation must stay below L / 2");
        const double side = p->L[a] / (double)ncell[a];
        FB_REQUIRE(ncell[a] >= 2 && side * side >= reach2[a], "pair counts: at least 2 cells per axis, of side >= the largest separation");
        ncells *= (unsigned long long)ncell[a];
        FB_REQUIRE(ncells <= (1ull << 31), "pair counts: at most 2^31 cells");
    }
    const PairWork w = pair_layout((unsigned long long)n1, (unsigned long long)n2, ncells);
    FB_REQUIRE(work_bytes >= (int64_t)w.total, "pair counts: work buffer smaller than fb_pair_work_bytes");
    FB_REQUIRE((n1 == 0 || pos1) && (n2 == 0 || pos2), "null pointer");
    *bad = 0;
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.0;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    char* wb = (char*)work;
    PairSmall* sm = (PairSmall*)wb;
    double* e2d = (double*)(wb + w.e2);
    unsigned *csum = (unsigned*)(wb + w.csum), *items = (unsigned*)(wb + w.items);
    const FofGeom g = geom_of(p, ncell);
    const size_t nbins = (size_t)nr * (size_t)nsub;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (stage_ms) for (int q = 0; q < 4; ++q) FB_HIP(hipEventCreate(&ev[q]));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int q = 0; q < 4; ++q) if (e[q]) (void)hipEventDestroy(e[q]); } } evg{ev};
    if (stage_ms) FB_HIP(hipEventRecord(ev[0], s));
    FB_HIP(hipMemsetAsync(counts_out, 0, nbins * 8, s));
    FB_HIP(hipMemsetAsync(sm, 0, FB_PAIR_SMALL, s));
    FB_HIP(hipMemcpyAsync(e2d, edges2, (size_t)(nr + 1) * 8, hipMemcpyHostToDevice, s));
    // 1. bin both catalogues into the same cells; a bad position anywhere ends the call before any counting
    const double* pos[2] = {pos1, pos2};
    const unsigned long long n[2] = {(unsigned long long)n1, (unsigned long long)n2};
    const int ncat = autoc ? 1 : 2;
    for (int q = 0; q < ncat; ++q) {
        if (!n[q]) continue;
        unsigned *cursor = (unsigned*)(wb + w.cat[q].cursor), *cellid = (unsigned*)(wb + w.cat[q].cellid);
        FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
        hipLaunchKernelGGL(k_fof_bin, dim3(grid_for(n[q], p)), dim3(256), 0, s, pos[q], n[q], g, cellid, cursor, &sm->err);
        FB_LAUNCH_CHECK("k_fof_bin");
    }
    PairSmall h;
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));   // (the edges have been read by now, too)
    if (h.err & FB_FOF_ERR_POS) { *bad = 1; return FB_OK; }
    if (n1 == 0 || (!autoc && n2 == 0)) return FB_OK;                 // no pair: the counts are zero
    for (int q = 0; q < ncat; ++q) {
        unsigned *start = (unsigned*)(wb + w.cat[q].start), *cursor = (unsigned*)(wb + w.cat[q].cursor),
                 *cellid = (unsigned*)(wb + w.cat[q].cellid);
        double* spos = (double*)(wb + w.cat[q].spos);
        const int rs = exscan(ScanPlain{cursor}, ncells, csum, start, s);       // start[ncells] = n[q]
        if (rs) return rs;
        FB_HIP(hipMemsetAsync(cursor, 0, (size_t)ncells * 4, s));
        hipLaunchKernelGGL(k_fof_scatter, dim3(grid_for(n[q], p)), dim3(256), 0, s, pos[q], n[q], g, (const unsigned*)cellid,
                           (const unsigned*)start, cursor, (unsigned*)nullptr, spos, (unsigned*)nullptr);
        FB_LAUNCH_CHECK("k_fof_scatter");
    }
    const unsigned* hstart = (const unsigned*)(wb + w.cat[0].start);
    const double* hpos = (const double*)(wb + w.cat[0].spos);
    const unsigned* nstart = autoc ? hstart : (const unsigned*)(wb + w.cat[1].start);
    const double* npos = autoc ? hpos : (const double*)(wb + w.cat[1].spos);
    hipLaunchKernelGGL(k_fof_items, dim3(grid_for(ncells, p)), dim3(256), 0, s, hstart, ncells, items, &sm->items);
    FB_LAUNCH_CHECK("k_fof_items");
    if (stage_ms) FB_HIP(hipEventRecord(ev[1], s));
    FB_TRY(fb_read_back(&h, sm, sizeof(h), s));
    const unsigned long long nitems = h.items;
    // 2. the sweep: tile 0 of every cell, then the further tiles of the crowded cells
    PairBins pb;
    pb.mode = mode; pb.nr = nr; pb.nsub = nsub;
    pb.rsteps = ceil_log2(nr); pb.ssteps = ceil_log2(nsub);
    pb.copies_log2 = 0;
    while (pb.copies_log2 < 6 && (nbins << (pb.copies_log2 + 1)) <= FB_PAIR_MAX_BINS) ++pb.copies_log2;
    pb.flush = g_pair_flush;
    pb.sub_a = mode == 1 ? (double)nsub * (double)nsub : 1.0;
    pb.sub_max2 = mode == 2 ? sub_max * sub_max : 0.0;
    const int self_mode = !autoc ? 0 : (ncell[0] >= 3 && ncell[1] >= 3 && ncell[2] >= 3 ? 1 : 2);
    const unsigned long long wgmax = 64ull * (unsigned long long)p->num_cu;
    hipLaunchKernelGGL(k_pair_sweep, dim3((unsigned)std::min(ncells, wgmax)), dim3(FB_PAIR_WG), 0, s, g, hstart, hpos, nstart, npos,
                       (const double*)e2d, pb, self_mode, (const unsigned*)nullptr, ncells, (unsigned long long*)counts_out);
    FB_LAUNCH_CHECK("k_pair_sweep");
    if (stage_ms) FB_HIP(hipEventRecord(ev[2], s));
    if (nitems) {
        hipLaunchKernelGGL(k_pair_sweep, dim3((unsigned)std::min(nitems, wgmax)), dim3(FB_PAIR_WG), 0, s, g, hstart, hpos, nstart, npos,
                           (const double*)e2d, pb, self_mode, (const unsigned*)items, nitems, (unsigned long long*)counts_out);
        FB_LAUNCH_CHECK("k_pair_sweep");
    }
    if (stage_ms) {
        FB_HIP(hipEventRecord(ev[3], s));
        FB_HIP(hipEventSynchronize(ev[3]));
        for (int q = 0; q < 3; ++q) {
            float ms = 0.f;
            FB_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            stage_ms[q] = (double)ms;
        }
    }
    return FB_OK;
}

}  // extern "C"
