// Two estimators that bin the transverse modes (m_x, m_y) in k_perp and keep the line of sight resolved: the cylindrical power
// spectrum P(k_perp, k_par) from one or two stored half spectra, and the multi-frequency angular power spectrum
// C(k_perp; nu, nu') -- a Gram matrix of the channels per k_perp bin on the fp64 matrix cores -- from one or two cubes
// transformed over their transverse axes.  Both plan precisions are compiled here; see include/fastbox_hip.h for the
// definitions and DESIGN.md section 4 for the algorithm and its limits.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"                      // mode_of
#include "fb_fft.h"                      // cx<T>
#include "fb_kshell.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace fb {
namespace {

#define FB_CYL_MAX_PERP 1024     // k_perp bins of fb_bin_power_cyl: the default edges of a 2048^3 box
#define FB_CYL_MAX_PAR 1025      // k_par bins: one per |m_z| of a 2048^3 box
#define FB_MAPS_MAX_BINS 256     // k_perp bins of fb_transverse_gram
#define FB_MAPS_MAX_N 1024

inline double host_sq2(double a, double b) {
#pragma clang fp contract(off)
    return a * a + b * b;
}

int cyl_rows_get(fb_plan* p, const double* edges, int nb, bool skip0, const fb_cyl_rows** out) {
    std::vector<double> key(edges, edges + nb + 1);
    key.push_back(skip0 ? 1.0 : 0.0);
    if ((*out = p->cyl_rows.find(key))) return FB_OK;
    const int N = p->N;
    double kf[3];
    fill_kf(p, kf);
    std::vector<double> kx(N), ky(N);
    for (int i = 0; i < N; ++i) {
        const int m = i < (N >> 1) ? i : i - N;
        kx[i] = (double)m * kf[0];
        ky[i] = (double)m * kf[1];
    }
    std::vector<short> bin((size_t)N * N);
    std::vector<int> off(nb + 1, 0);
    std::vector<long double> sk(nb, 0.0L);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const double k = std::sqrt(host_sq2(kx[i], ky[j]));
            int b = (int)(std::upper_bound(edges, edges + nb + 1, k) - edges) - 1;      // np.digitize(k, edges) - 1
            if (b >= nb || (skip0 && i == 0 && j == 0)) b = -1;
            bin[(size_t)i * N + j] = (short)b;
            if (b >= 0) { ++off[b + 1]; sk[b] += (long double)k; }
        }
    for (int b = 0; b < nb; ++b) off[b + 1] += off[b];
    std::vector<int> rows(std::max(off[nb], 1)), next(off.begin(), off.end() - 1);
    for (int r = 0; r < N * N; ++r) if (bin[r] >= 0) rows[next[bin[r]]++] = r;
    fb_cyl_rows e;
    e.nb = nb; e.off = off;
    e.sumk.resize(nb);
    for (int b = 0; b < nb; ++b) e.sumk[b] = (double)sk[b];
    e.has0 = bin[0] >= 0;
    FB_TRY(e.rows_dev.ensure(rows.size() * sizeof(int)));
    FB_HIP(hipMemcpy(e.rows_dev, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
    // (a full cache drops its oldest list here; every entry point synchronises: no launch still reads it)
    *out = p->cyl_rows.insert(std::move(key), std::move(e));
    return FB_OK;
}

// chunks of at most rc rows, none across a bin boundary: tab[3 c] = (bin, first row, one past the last); choff[b] = the first
// chunk of bin b
void make_chunks(const fb_cyl_rows& e, long long rc, std::vector<int>& tab, std::vector<int>& choff) {
    tab.clear();
    choff.assign(e.nb + 1, 0);
    for (int b = 0; b < e.nb; ++b) {
        choff[b] = (int)(tab.size() / 3);
        for (long long r = e.off[b]; r < e.off[b + 1]; r += rc) {
            tab.push_back(b); tab.push_back((int)r); tab.push_back((int)std::min<long long>(r + rc, e.off[b + 1]));
        }
    }
    choff[e.nb] = (int)(tab.size() / 3);
}

// ---- cylindrical power ------------------------------------------------------------------------------------------------------
// In the stored half spectrum m_z is the fastest axis: a whole (m_x, m_y) row lies in one k_perp bin and its k_par bin depends
// on m_z alone.  A workgroup owns one chunk of a bin's rows and a tile of 64 m_z: its four waves take the chunk's rows four at
// a time (every load a 64-lane run along m_z), each lane sums Re(conj(D_1) D_2) of its m_z in fp64 in four chains, the waves
// are added in order and the workgroup writes partial[chunk][m_z].  No LDS table of cells: any number of (k_perp, k_par) cells.
struct CylArgs {
    const int* rows;
    const int* chunks;
    int N, NZV, NZP, NR;
};

template <typename T>
__global__ __launch_bounds__(256) void k_cyl_rows(const cx<T>* __restrict__ h1, const cx<T>* __restrict__ h2,
                                                  double* __restrict__ partial, CylArgs a) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.x, l = blockIdx.y * 64 + lane;
    const int r0 = a.chunks[3 * chunk + 1], r1 = a.chunks[3 * chunk + 2];
    const bool in = l < a.NZV;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + 4 * wave; r < r1; r += 16) {
        cx<T> d1[4], d2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                                  // all loads of the four rows first
            const bool ok = in && r + u < r1;
            const int row = a.rows[r + u < r1 ? r + u : r0];
            const long long at = ((long long)(row / a.N) * a.NR + row % a.N) * a.NZP + l;
            const bool use = ok && (row | l) != 0;                     // k = 0 is excluded
            d1[u] = use ? h1[at] : cx<T>{0, 0};
            d2[u] = (h2 && use) ? h2[at] : d1[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (double)d1[u].x * (double)d2[u].x + (double)d1[u].y * (double)d2[u].y;
    }
    sh[wave][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (wave == 0 && in) partial[(size_t)chunk * a.NZV + l] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

// One workgroup per k_perp bin: S(b, m_z) = the bin's chunks added in order, times the weight of the plane (m_z = 0 and N/2
// once, the others twice); then the k_par cell c sums its m_z in [lr[2 c], lr[2 c + 1]) in order.
__global__ __launch_bounds__(256) void k_cyl_finish(const double* __restrict__ partial, const int* __restrict__ choff,
                                                    const int* __restrict__ lr, int NZV, int N, int npar, double scale,
                                                    double* __restrict__ out) {
    __shared__ double s[FB_CYL_MAX_PAR];
    const int b = blockIdx.x, c0 = choff[b], c1 = choff[b + 1];
    for (int l = threadIdx.x; l < NZV; l += blockDim.x) {
        double t = 0.0;
        for (int c = c0; c < c1; ++c) t += partial[(size_t)c * NZV + l];
        s[l] = ((l == 0 || 2 * l == N) ? 1.0 : 2.0) * t;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < npar; c += blockDim.x) {
        double t = 0.0;
        for (int l = lr[2 * c]; l < lr[2 * c + 1]; ++l) t += s[l];
        out[(size_t)b * npar + c] = t * scale;
    }
}

int cyl_check(const fb_plan* p, const double* pe, int nperp, const double* qe, int npar) {
    FB_REQUIRE(nperp >= 1 && nperp <= FB_CYL_MAX_PERP, "nperp must be in 1..1024");
    FB_REQUIRE(npar >= 1 && npar <= FB_CYL_MAX_PAR, "npar must be in 1..1025");
    const int r = kshell_check_edges(pe, nperp);
    if (r) return r;
    for (int q = 0; q < npar; ++q) FB_REQUIRE(std::isfinite(qe[q]), "k_par edges must be finite (the last may be inf)");
    for (int q = 1; q <= npar; ++q) FB_REQUIRE(qe[q] > qe[q - 1], "k_par edges must be strictly ascending");
    return FB_OK;
}

int bin_power_cyl(fb_plan* p, const void* half1, const void* half2, const double* pe, int nperp, const double* qe, int npar,
                  double* out_host, hipStream_t s) {
    const int N = p->N, NZV = p->NZV;
    const fb_cyl_rows* e = nullptr;
    int r = cyl_rows_get(p, pe, nperp, false, &e);
    if (r) return r;
    // k_par = |k_z| grows with m_z: a k_par cell is a run of m_z
    double kf[3];
    fill_kf(p, kf);
    std::vector<int> lr(2 * (size_t)npar, 0);
    std::vector<long double> wsum(npar, 0.0L), wk(npar, 0.0L);
    int c0 = -1;                                                       // the cell of m_z = 0
    for (int l = 0; l < NZV; ++l) {
        const double kz = (double)l * kf[2];
        const int c = (int)(std::upper_bound(qe, qe + npar + 1, kz) - qe) - 1;     // np.digitize(|k_z|, par_edges) - 1
        if (c < 0 || c >= npar) continue;
        if (lr[2 * c + 1] == 0) lr[2 * c] = l;
        lr[2 * c + 1] = l + 1;
        const long double w = (l == 0 || 2 * l == N) ? 1.0L : 2.0L;
        wsum[c] += w; wk[c] += w * (long double)kz;
        if (l == 0) c0 = c;
    }
    // rows of a chunk: about 1024 chunks over the plane, at least 32 rows
    const long long rc = std::max(32LL, ((long long)N * N + 1023) / 1024);
    std::vector<int> tab, choff;
    make_chunks(*e, rc, tab, choff);
    const int nch = (int)(tab.size() / 3);
    std::vector<int> idx(tab);
    idx.insert(idx.end(), choff.begin(), choff.end());
    idx.insert(idx.end(), lr.begin(), lr.end());
    r = p->cyl_idx.ensure(idx.size() * sizeof(int));
    if (!r) r = p->cyl_partials.ensure((size_t)std::max(nch, 1) * NZV * sizeof(double));
    if (!r) r = p->cyl_tab.ensure((size_t)nperp * npar * sizeof(double));
    if (r) return r;
    double* sums_dev = p->cyl_tab;                                     // [nperp][npar] sum P
    FB_HIP(hipMemcpyAsync(p->cyl_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, s));
    CylArgs a;
    a.rows = e->rows_dev; a.chunks = p->cyl_idx; a.N = N; a.NZV = NZV; a.NZP = p->NZP; a.NR = p->NR;
    if (nch > 0) {
        FbProfScope _ps(p, FBK_BIN, s);
        const dim3 grid(nch, (NZV + 63) / 64);
        if (p->prec == 4) hipLaunchKernelGGL((k_cyl_rows<float>), grid, dim3(256), 0, s, (const cx<float>*)half1,
                                             (const cx<float>*)half2, p->cyl_partials, a);
        else hipLaunchKernelGGL((k_cyl_rows<double>), grid, dim3(256), 0, s, (const cx<double>*)half1,
                                (const cx<double>*)half2, p->cyl_partials, a);
    }
    FB_LAUNCH_CHECK("k_cyl_rows");
    // P = (Lx Ly Lz / N^6) Re(conj(D_1) D_2)
    const double n3 = (double)N * N * N;
    const double scale = (p->L[0] * p->L[1] * p->L[2]) / (n3 * n3);
    { FbProfScope _ps(p, FBK_BIN, s);
    hipLaunchKernelGGL(k_cyl_finish, dim3(nperp), dim3(256), 0, s, p->cyl_partials.as<const double>(), p->cyl_idx + 3 * nch,
                       p->cyl_idx + 3 * nch + nperp + 1, NZV, N, npar, scale, sums_dev); }
    FB_LAUNCH_CHECK("k_cyl_finish");
    const size_t nc = (size_t)nperp * npar;
    FB_HIP(hipMemcpyAsync(out_host + 3 * nc, sums_dev, nc * sizeof(double), hipMemcpyDeviceToHost, s));
    // the data-independent sums: a cell holds every row of its k_perp bin at every m_z of its run
    for (int b = 0; b < nperp; ++b) {
        const long double nrow = (long double)(e->off[b + 1] - e->off[b]);
        for (int c = 0; c < npar; ++c) {
            const size_t q = (size_t)b * npar + c;
            long double modes = nrow * wsum[c];
            if (b == 0 && c == c0 && e->has0) modes -= 1.0L;           // k = 0 (it adds 0 to both wavenumber sums)
            out_host[q] = (double)modes;
            out_host[nc + q] = (double)((long double)e->sumk[b] * wsum[c]);
            out_host[2 * nc + q] = (double)(nrow * wk[c]);
        }
    }
    FB_HIP(hipStreamSynchronize(s));
    return FB_OK;
}

// ---- multi-frequency angular power ------------------------------------------------------------------------------------------
// Re(a conj(a')) = Re a Re a' + Im a Im a': per k_perp bin a real Gram matrix over the channels whose rows are the (mode,
// re / im) pairs of the bin -- the contraction of k_channel_cov (fb_field_kernels.h) with the rows gathered through the sorted
// list.  A rank-4 update of v_mfma_f64_16x16x4_f64 takes four modes: lane l loads the complex value of mode p + (l >> 4),
// channel a0 + (l & 15) once and feeds its real part to one matrix instruction and its imaginary part to the next.  One wave
// owns a (16 MA)^2 block of the matrix for one chunk of one bin's modes (a chunk never crosses a bin boundary; the last update
// of a chunk is masked where the count is no multiple of 4).  Auto: blocks bi <= bj only, B from the same cube; cross: every
// block, A from cube 1 (rows of the result) and B from cube 2 (columns).  partial[chunk][nu][nu'], added per bin in chunk order
// by k_maps_finish.  EDGE as at k_channel_cov: channels past N read channel N - 1, count as 0 and are not stored.
typedef double fb_d4 __attribute__((ext_vector_type(4)));

template <typename T, int MA, bool EDGE>
__global__ __launch_bounds__(64) void k_maps_gram(const cx<T>* __restrict__ c1, const cx<T>* __restrict__ c2,
                                                  const int* __restrict__ rows, const int* __restrict__ chunks,
                                                  double* __restrict__ partial, int N, int nbs, int cross) {
    int bi = 0, bj;
    if (cross) { bi = blockIdx.x / nbs; bj = blockIdx.x % nbs; }
    else {
        int rem = blockIdx.x;
        while (rem >= nbs - bi) { rem -= nbs - bi; ++bi; }
        bj = bi + rem;
    }
    const int lane = threadIdx.x, lc = lane & 15, lk = lane >> 4;
    const int a0 = bi * 16 * MA, b0 = bj * 16 * MA;
    const int chunk = blockIdx.y;
    const int p0 = chunks[3 * chunk + 1], p1 = chunks[3 * chunk + 2];
    int ca[MA], cb[MA];
    bool oka[MA], okb[MA];
#pragma unroll
    for (int i = 0; i < MA; ++i) {
        ca[i] = a0 + 16 * i + lc; cb[i] = b0 + 16 * i + lc;
        oka[i] = !EDGE || ca[i] < N; okb[i] = !EDGE || cb[i] < N;
        if (EDGE) { ca[i] = ca[i] < N ? ca[i] : N - 1; cb[i] = cb[i] < N ? cb[i] : N - 1; }
    }
    fb_d4 acc[MA][MA];
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int j = 0; j < MA; ++j) acc[i][j] = fb_d4{0.0, 0.0, 0.0, 0.0};
    // the software pipeline of k_channel_cov: the operands of the next KU updates are fetched before the matrix instructions
    // of the current ones are issued (KU = 2 at MA = 4: a complex operand takes twice the registers of a real one)
    constexpr int KU = MA == 4 ? 2 : 4;
    cx<T> fa[2][KU][MA], fb_[2][KU][MA];
    auto fetch = [&](int buf, int p) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int m = p + 4 * u + lk;
            const size_t row = (size_t)rows[m < p1 ? m : p0] * N;   // past the chunk: any valid mode, masked below
#pragma unroll
            for (int i = 0; i < MA; ++i) { fa[buf][u][i] = c1[row + ca[i]]; fb_[buf][u][i] = c2[row + cb[i]]; }
        }
    };
    auto update = [&](int buf, int p) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const bool ok = p + 4 * u + lk < p1;
            double ar[MA], ai[MA], br[MA], bi_[MA];
#pragma unroll
            for (int i = 0; i < MA; ++i) {
                ar[i] = (ok && oka[i]) ? (double)fa[buf][u][i].x : 0.0;
                ai[i] = (ok && oka[i]) ? (double)fa[buf][u][i].y : 0.0;
                br[i] = (ok && okb[i]) ? (double)fb_[buf][u][i].x : 0.0;
                bi_[i] = (ok && okb[i]) ? (double)fb_[buf][u][i].y : 0.0;
            }
#pragma unroll
            for (int i = 0; i < MA; ++i)
#pragma unroll
                for (int j = 0; j < MA; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], bi_[j], acc[i][j], 0, 0, 0);
                }
        }
    };
    fetch(0, p0);
    for (int p = p0; p < p1; p += 8 * KU) {
        fetch(1, p + 4 * KU);
        update(0, p);
        if (p + 4 * KU < p1) {
            fetch(0, p + 8 * KU);
            update(1, p + 4 * KU);
        }
    }
    double* dst = partial + (size_t)chunk * N * N;
#pragma unroll
    for (int i = 0; i < MA; ++i)
#pragma unroll
        for (int j = 0; j < MA; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (!EDGE || (a0 + 16 * i + lk + 4 * r < N && b0 + 16 * j + lc < N))
                    dst[(size_t)(a0 + 16 * i + lk + 4 * r) * N + b0 + 16 * j + lc] = acc[i][j][r];
}

// cl[b][nu][nu'] = inv[b] (the bin's chunks added in order), inv[b] = Lx Ly / (N^4 modes_b), NaN for an empty bin.  sym (auto):
// the element with nu <= nu' is formed and written to both places, so the result is symmetric bit for bit.
__global__ __launch_bounds__(64) void k_maps_finish(const double* __restrict__ partial, const int* __restrict__ choff,
                                                    const double* __restrict__ inv, int N, int sym, double* __restrict__ cl) {
    const int c = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y, b = blockIdx.z;
    if (c >= N || (sym && a > c)) return;
    double s = 0.0;
    for (int q = choff[b]; q < choff[b + 1]; ++q) s += partial[((size_t)q * N + a) * N + c];
    s *= inv[b];
    cl[((size_t)b * N + a) * N + c] = s;
    if (sym && a != c) cl[((size_t)b * N + c) * N + a] = s;
}

struct GramShape { int MA, bs, nbs, npairs, slices; bool edge; };
// blocks of 16 MA channels as fbi_channel_cov chooses them; about 8 waves per CU over all chunks
GramShape gram_shape(const fb_plan* p, bool cross) {
    GramShape g;
    const int N = p->N;
    g.MA = N % 64 == 0 ? 4 : (N % 32 == 0 ? 2 : 1);
    g.edge = N % 16 != 0;
    g.bs = 16 * g.MA;
    g.nbs = (N + g.bs - 1) / g.bs;
    g.npairs = cross ? g.nbs * g.nbs : g.nbs * (g.nbs + 1) / 2;
    g.slices = std::max(1, (8 * p->num_cu + g.npairs - 1) / g.npairs);
    return g;
}

template <typename T>
void gram_launch(const GramShape& g, dim3 grid, hipStream_t s, const void* c1, const void* c2, const int* rows, const int* chunks,
                 double* partial, int N, int cross) {
    const cx<T>* x1 = (const cx<T>*)c1;
    const cx<T>* x2 = (const cx<T>*)c2;
    if (g.MA == 4) hipLaunchKernelGGL((k_maps_gram<T, 4, false>), grid, dim3(64), 0, s, x1, x2, rows, chunks, partial, N, g.nbs, cross);
    else if (g.MA == 2) hipLaunchKernelGGL((k_maps_gram<T, 2, false>), grid, dim3(64), 0, s, x1, x2, rows, chunks, partial, N, g.nbs, cross);
    else if (!g.edge) hipLaunchKernelGGL((k_maps_gram<T, 1, false>), grid, dim3(64), 0, s, x1, x2, rows, chunks, partial, N, g.nbs, cross);
    else hipLaunchKernelGGL((k_maps_gram<T, 1, true>), grid, dim3(64), 0, s, x1, x2, rows, chunks, partial, N, g.nbs, cross);
}

int maps_check(const fb_plan* p, const double* edges, int nb) {
    FB_REQUIRE(p->N <= FB_MAPS_MAX_N, "the angular power spectrum takes grids up to 1024^3");
    FB_REQUIRE(nb >= 1 && nb <= FB_MAPS_MAX_BINS, "nb must be in 1..256");
    return kshell_check_edges(edges, nb);
}

int transverse_gram(fb_plan* p, const void* full1, const void* full2, const double* edges, int nb, double* cl_dev,
                    void* work_dev, double* out_host, hipStream_t s) {
    const int N = p->N;
    const bool cross = full2 != nullptr;
    const fb_cyl_rows* e = nullptr;
    int r = cyl_rows_get(p, edges, nb, true, &e);
    if (r) return r;
    const GramShape g = gram_shape(p, cross);
    // rows of a chunk: the listed modes over `slices` chunks, whole rank-4 updates, at least 16 modes
    long long rc = ((long long)e->off[nb] + g.slices - 1) / g.slices;
    rc = std::max(16LL, (rc + 3) & ~3LL);
    std::vector<int> tab, choff;
    make_chunks(*e, rc, tab, choff);
    const int nch = (int)(tab.size() / 3);                            // <= slices + nb: fb_transverse_gram_work_bytes
    std::vector<int> idx(tab);
    idx.insert(idx.end(), choff.begin(), choff.end());
    const double n2 = (double)N * N;
    const double norm = (p->L[0] * p->L[1]) / (n2 * n2);
    std::vector<double> inv(nb);
    for (int b = 0; b < nb; ++b) {
        const double modes = (double)(e->off[b + 1] - e->off[b]);
        out_host[b] = modes;
        out_host[nb + b] = e->sumk[b];
        inv[b] = modes > 0.0 ? norm / modes : std::numeric_limits<double>::quiet_NaN();
    }
    r = p->cyl_idx.ensure(idx.size() * sizeof(int));
    if (!r) r = p->cyl_tab.ensure((size_t)nb * sizeof(double));
    if (r) return r;
    FB_HIP(hipMemcpyAsync(p->cyl_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, s));
    FB_HIP(hipMemcpyAsync(p->cyl_tab, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (nch > 0) {
        FbProfScope _ps(p, FBK_PCA, s);
        const dim3 grid(g.npairs, nch);
        const void* second = cross ? full2 : full1;
        if (p->prec == 4) gram_launch<float>(g, grid, s, full1, second, e->rows_dev, p->cyl_idx, (double*)work_dev, N, cross ? 1 : 0);
        else gram_launch<double>(g, grid, s, full1, second, e->rows_dev, p->cyl_idx, (double*)work_dev, N, cross ? 1 : 0);
    }
    FB_LAUNCH_CHECK("k_maps_gram");
    { FbProfScope _ps(p, FBK_PCA, s);
    hipLaunchKernelGGL(k_maps_finish, dim3((N + 63) / 64, N, nb), dim3(64), 0, s, (const double*)work_dev, p->cyl_idx + 3 * nch,
                       p->cyl_tab.as<const double>(), N, cross ? 0 : 1, cl_dev); }
    FB_LAUNCH_CHECK("k_maps_finish");
    FB_HIP(hipStreamSynchronize(s));
    return FB_OK;
}

}  // namespace
}  // namespace fb

extern "C" {

int fb_bin_power_cyl(fb_plan* p, const void* half1, const void* half2, const double* perp_edges, int nperp,
                     const double* par_edges, int npar, double* out_host, void* stream) {
    FB_REQUIRE(p && half1 && perp_edges && par_edges && out_host, "null pointer");
    const int r = fb::cyl_check(p, perp_edges, nperp, par_edges, npar);
    if (r) return r;
    FB_USE_DEVICE(p);
    return fb::bin_power_cyl(p, half1, half2, perp_edges, nperp, par_edges, npar, out_host, (hipStream_t)stream);
}

int fb_power_spectrum_cyl(fb_plan* p, const void* real1, const void* real2, void* work_half1, void* work_half2,
                          const double* perp_edges, int nperp, const double* par_edges, int npar, double* out_host,
                          void* stream) {
    FB_REQUIRE(p && real1 && work_half1 && perp_edges && par_edges && out_host, "null pointer");
    FB_REQUIRE(!real2 || work_half2, "a cross spectrum needs work_half2");
    int r = fb::cyl_check(p, perp_edges, nperp, par_edges, npar);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real1, work_half1, 0, s), fbi_fft_r2c_f64(p, real1, work_half1, 0, s));
    if (!r && real2) r = FB_DISPATCH(p, fbi_fft_r2c_f32(p, real2, work_half2, 0, s), fbi_fft_r2c_f64(p, real2, work_half2, 0, s));
    if (r) return r;
    return fb::bin_power_cyl(p, work_half1, real2 ? work_half2 : nullptr, perp_edges, nperp, par_edges, npar, out_host, s);
}

long long fb_transverse_gram_work_bytes(const fb_plan* p, int nb, int cross) {
    if (!p || nb < 1) return 0;
    const fb::GramShape g = fb::gram_shape(p, cross != 0);
    return (long long)(g.slices + nb) * p->N * p->N * (long long)sizeof(double);
}

int fb_transverse_gram(fb_plan* p, const void* full1, const void* full2, const double* perp_edges, int nb, double* cl_dev,
                       void* work_dev, double* out_host, void* stream) {
    FB_REQUIRE(p && full1 && perp_edges && cl_dev && work_dev && out_host, "null pointer");
    const int r = fb::maps_check(p, perp_edges, nb);
    if (r) return r;
    FB_USE_DEVICE(p);
    return fb::transverse_gram(p, full1, full2, perp_edges, nb, cl_dev, work_dev, out_host, (hipStream_t)stream);
}

int fb_angular_power(fb_plan* p, const void* real1, const void* real2, void* work_full1, void* work_full2,
                     const double* perp_edges, int nb, double* cl_dev, void* work_dev, double* out_host, void* stream) {
    FB_REQUIRE(p && real1 && work_full1 && perp_edges && cl_dev && work_dev && out_host, "null pointer");
    FB_REQUIRE(!real2 || work_full2, "a cross spectrum needs work_full2");
    int r = fb::maps_check(p, perp_edges, nb);
    if (r) return r;
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    const void* re[2] = {real1, real2};
    void* full[2] = {work_full1, work_full2};
    for (int q = 0; q < 2 && re[q]; ++q) {
        r = FB_DISPATCH(p, fbi_real_to_complex_f32(p, re[q], full[q], s), fbi_real_to_complex_f64(p, re[q], full[q], s));
        if (!r) r = FB_DISPATCH(p, fbi_fft_axes01_f32(p, full[q], -1, 1.0, s), fbi_fft_axes01_f64(p, full[q], -1, 1.0, s));
        if (r) return r;
    }
    return fb::transverse_gram(p, work_full1, real2 ? work_full2 : nullptr, perp_edges, nb, cl_dev, work_dev, out_host, s);
}

}  // extern "C"
