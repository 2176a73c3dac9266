// Model fits along the line of sight ("Line-of-sight foreground fits"): a weighted polynomial in a Legendre
// basis per line of sight (fb_los_polyfit), the bounded power-law fit and two-template solve of the reference's LSQfitting.do_loop
// (fastbox/filters.py:625-664; fb_los_powerlaw), and the elementwise finish of the Gaussian-process filter (fb_los_subtract; its
// product is fb_los_matmul of fb_inpaint.hip).  Entry points: include/fastbox_hip.h.
//
// The cube is T[pixel][channel], the channel contiguous; a line of sight is one row of the (N^2, N) view.  One wave owns one
// row: lane l holds channels l, l + 64, ... in registers (CPL of them, a template case), so the row is read from memory once and
// the result is written once.  All fit state is fp64 whatever the plan's precision.  Every sum is a lane partial in ascending
// channel order followed by an xor butterfly over the wave: no floating-point atomics, every lane ends with the same bits (the
// additions of a butterfly step commute), so the branches taken on those sums are uniform over the wave and results are bitwise
// repeatable.  Every loop has a bound that does not depend on the data.  A datum under a flag (w = 0) is selected away, never
// multiplied: NaN there is legal.  The small tables (basis values, ln x, the channel terms) are N to 8 N doubles read with the
// lane's own channel index: coalesced, and resident in L1 / L2 after the first workgroups.
#include "../../include/fastbox_hip.h"
#include "fb_plan.h"
#include "fb_api_util.h"
#include "fb_dev.h"
#include <cmath>

#define FB_LOSFIT_NMAX 1024              // channels: 16 per lane
#define FB_LOSFIT_KMAX 8                 // coefficients: order 0 .. 7
#define FB_LOSFIT_ROWS 4                 // rows (waves) per workgroup

namespace {
using namespace fb;

// w or sigma of voxel (p, c): NULL counts as 1, else double[N] on the device (FB_GCR_PER_CHANNEL) or a cube in the plan's
// precision (FB_GCR_PER_VOXEL)
template <typename T>
__device__ __forceinline__ double aux_at(const void* a, int kind, long long i, int c) {
    if (!a) return 1.0;
    return kind == FB_GCR_PER_CHANNEL ? ((const double*)a)[c] : (double)((const T*)a)[i];
}
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }     // false for NaN
// a decision every lane takes alike, told to the compiler
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ constexpr int tri(int k, int l) { return k * (k + 1) / 2 + l; }              // l <= k

// ---- polynomial fit ---------------------------------------------------------------------------------------------------------------
struct PolyArgs {
    const void* cube;
    const void* w;
    int w_kind;
    const double* basis;        // [K1][N]: P_k(t_c)
    const double* pinv;         // [K1][N]: the shared pseudo-inverse with w folded in (coefficient k = sum_c pinv[k][c] y_c), or NULL
    int K1;                     // order + 1
    int logy;                   // y = ln T, model = exp(fit)
    void* out;
    void* model;                // may be NULL
    double* coeffs;             // [K1][npix], may be NULL
    double* chi2;               // [npix], may be NULL
    int32_t* status;            // [npix]
    int* n_failed;
    long long npix;
    int N;
};

template <typename T, int CPL>
__global__ __launch_bounds__(64 * FB_LOSFIT_ROWS) void k_los_polyfit(const PolyArgs a) {
    const int lane = threadIdx.x & 63, N = a.N, K1 = a.K1;
    const long long p = (long long)blockIdx.x * FB_LOSFIT_ROWS + (threadIdx.x >> 6);
    if (p >= a.npix) return;                                   // wave-uniform; the kernel has no barrier
    const T* row = (const T*)a.cube + p * N;
    const bool logy = a.logy != 0;
    double tv[CPL], w2[CPL];
    int cnt = 0, nonfinite = 0, nonpos = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < N;
        const double wv = in ? aux_at<T>(a.w, a.w_kind, p * N + c, c) : 0.0;
        const bool good = in && wv != 0.0;
        const double t = in ? (double)row[c] : 0.0;
        tv[j] = good ? t : 0.0;
        w2[j] = good ? wv * wv : 0.0;
        cnt += __popcll(__ballot(good));
        nonfinite |= __any(good && !finite_d(t));
        nonpos |= __any(good && logy && t <= 0.0);
    }
    int status = cnt < K1 ? FB_LOSFIT_TOO_FEW : (nonfinite ? FB_LOSFIT_NONFINITE : (nonpos ? FB_LOSFIT_NONPOSITIVE : FB_LOSFIT_OK));
    status = uniform(status);
    double coef[FB_LOSFIT_KMAX];
#pragma unroll
    for (int k = 0; k < FB_LOSFIT_KMAX; ++k) coef[k] = 0.0;
    if (status == FB_LOSFIT_OK && a.pinv) {
        // one shared pseudo-inverse: K1 sums
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            if (64 * j < N) {
                const double y = w2[j] != 0.0 ? (logy ? log(tv[j]) : tv[j]) : 0.0;
#pragma unroll
                for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                    if (k < K1) coef[k] += (c < N && w2[j] != 0.0) ? a.pinv[(size_t)k * N + c] * y : 0.0;
            }
        }
#pragma unroll
        for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
            if (k < K1) coef[k] = wave_sum(coef[k]);
    } else if (status == FB_LOSFIT_OK) {
        // this row's own normal equations (lower triangle) and right-hand side
        double Am[FB_LOSFIT_KMAX * (FB_LOSFIT_KMAX + 1) / 2], bv[FB_LOSFIT_KMAX];
#pragma unroll
        for (int i = 0; i < FB_LOSFIT_KMAX * (FB_LOSFIT_KMAX + 1) / 2; ++i) Am[i] = 0.0;
#pragma unroll
        for (int k = 0; k < FB_LOSFIT_KMAX; ++k) bv[k] = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            if (64 * j < N) {
                const double ww = w2[j];
                const double y = ww != 0.0 ? (logy ? log(tv[j]) : tv[j]) : 0.0;
                double pv[FB_LOSFIT_KMAX];
#pragma unroll
                for (int k = 0; k < FB_LOSFIT_KMAX; ++k) pv[k] = (k < K1 && c < N) ? a.basis[(size_t)k * N + c] : 0.0;
#pragma unroll
                for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                    if (k < K1) {
                        const double wp = ww * pv[k];
                        bv[k] += wp * y;
#pragma unroll
                        for (int l = 0; l <= k; ++l) Am[tri(k, l)] += wp * pv[l];
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
            if (k < K1) {
                bv[k] = wave_sum(bv[k]);
#pragma unroll
                for (int l = 0; l <= k; ++l) Am[tri(k, l)] = wave_sum(Am[tri(k, l)]);
            }
        // Cholesky A = L L^T in place, row by row; every lane does the same arithmetic on the same bits
        int ok = 1;
#pragma unroll
        for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
            if (k < K1) {
#pragma unroll
                for (int l = 0; l <= k; ++l) {
                    double s = Am[tri(k, l)];
#pragma unroll
                    for (int m = 0; m < l; ++m) s -= Am[tri(k, m)] * Am[tri(l, m)];
                    if (l < k) Am[tri(k, l)] = s / Am[tri(l, l)];
                    else { if (!(s > 0.0) || !finite_d(s)) ok = 0; Am[tri(k, k)] = sqrt(s); }
                }
            }
        auto solve = [&](double (&v)[FB_LOSFIT_KMAX]) {                     // v <- (L L^T)^-1 v
#pragma unroll
            for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                if (k < K1) {
                    double s = v[k];
#pragma unroll
                    for (int m = 0; m < k; ++m) s -= Am[tri(k, m)] * v[m];
                    v[k] = s / Am[tri(k, k)];
                }
#pragma unroll
            for (int k = FB_LOSFIT_KMAX - 1; k >= 0; --k)
                if (k < K1) {
                    double s = v[k];
#pragma unroll
                    for (int m = k + 1; m < FB_LOSFIT_KMAX; ++m)
                        if (m < K1) s -= Am[tri(m, k)] * v[m];
                    v[k] = s / Am[tri(k, k)];
                }
        };
        if (!uniform(ok)) status = FB_LOSFIT_SINGULAR;
        else {
#pragma unroll
            for (int k = 0; k < FB_LOSFIT_KMAX; ++k) coef[k] = bv[k];
            solve(coef);
            // One step of refinement with the residual taken from the data (the corrected semi-normal equations): the
            // normal matrix squares the condition of the design, and a line of sight that keeps few channels can reach 1e3;
            // a += (L L^T)^-1 P^T w^2 (y - P a) brings the error back to that of a QR solve.
#pragma unroll
            for (int k = 0; k < FB_LOSFIT_KMAX; ++k) bv[k] = 0.0;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int c = lane + 64 * j;
                if (64 * j < N) {
                    const double ww = w2[j];
                    double r = ww != 0.0 ? (logy ? log(tv[j]) : tv[j]) : 0.0;
                    double pv[FB_LOSFIT_KMAX];
#pragma unroll
                    for (int k = 0; k < FB_LOSFIT_KMAX; ++k) {
                        pv[k] = (k < K1 && c < N) ? a.basis[(size_t)k * N + c] : 0.0;
                        r -= coef[k] * pv[k];
                    }
                    r *= ww;
#pragma unroll
                    for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                        if (k < K1) bv[k] += pv[k] * r;
                }
            }
#pragma unroll
            for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                if (k < K1) bv[k] = wave_sum(bv[k]);
            solve(bv);
#pragma unroll
            for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                if (k < K1) coef[k] += bv[k];
        }
    }
    // the model at every channel, the residual where w != 0
    T* orow = (T*)a.out + p * N;
    T* mrow = a.model ? (T*)a.model + p * N : nullptr;
    double chi = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        if (c < N) {
            if (status != FB_LOSFIT_OK) {
                orow[c] = (T)NAN;
                if (mrow) mrow[c] = (T)NAN;
            } else {
                double fit = 0.0;
#pragma unroll
                for (int k = 0; k < FB_LOSFIT_KMAX; ++k)
                    if (k < K1) fit += coef[k] * a.basis[(size_t)k * N + c];
                const double m = logy ? exp(fit) : fit;
                const bool good = w2[j] != 0.0;
                if (good) {
                    const double r = (logy ? log(tv[j]) : tv[j]) - fit;
                    chi += w2[j] * r * r;
                }
                orow[c] = good ? (T)(tv[j] - m) : (T)0;
                if (mrow) mrow[c] = (T)m;
            }
        }
    }
    chi = wave_sum(chi);
    if (lane == 0) {
        a.status[p] = status;
        if (a.chi2) a.chi2[p] = status == FB_LOSFIT_OK ? chi : NAN;
        if (a.coeffs)
            for (int k = 0; k < K1; ++k) a.coeffs[(size_t)k * a.npix + p] = status == FB_LOSFIT_OK ? coef[k] : NAN;
        if (status != FB_LOSFIT_OK) atomicAdd(a.n_failed, 1);          // an integer count: the order does not matter
    }
}

// ---- power-law fit ----------------------------------------------------------------------------------------------------------------
struct PlawArgs {
    const void* maps;
    const double* tpsmean;      // [N] or NULL
    const void* sigma;
    int s_kind;
    const void* w;
    int w_kind;
    const double* lnx;          // [N]: ln(nu_c / nu_0)
    double freeind;
    const double* beta_guess;   // [npix] or NULL
    int max_iter;
    double tol;
    void* resid;
    void* model;                // may be NULL
    double* rows;               // [5][npix]: betaS, ampS, syamp, ffamp, cost
    int32_t* n_iter;
    int32_t* status;
    int* n_failed;
    long long npix;
    int N;
};

// The projected functional at beta: g = q x^beta, h = q d, ampS = clip(g.h / g.g) (the exact minimiser over its interval: the
// cost is a convex parabola in ampS), r = ampS g - h, cost = r.r / 2, and the Gauss-Newton step of beta on it -- with ampS free
// the step of the two-parameter normal equations with ampS eliminated, with ampS on a bound the one-parameter step.
// ok = 0 where a denominator is not positive or a sum is not finite.
template <int CPL>
struct PlawRow {
    double d[CPL], q[CPL], lx[CPL], g[CPL];
    int N;
    double alo, ahi;
    __device__ __forceinline__ void eval(double beta, double& amp, double& cost, double& step, int& ok) {
        double gg = 0.0, gh = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (64 * j < N) {
                g[j] = q[j] != 0.0 ? q[j] * exp(beta * lx[j]) : 0.0;
                gg += g[j] * g[j];
                gh += g[j] * (q[j] * d[j]);
            }
        gg = wave_sum(gg); gh = wave_sum(gh);
        const double free_amp = gh / gg;
        amp = free_amp < alo ? alo : (free_amp > ahi ? ahi : free_amp);
        const bool clipped = amp != free_amp;
        double rr = 0.0, jr = 0.0, jj = 0.0, gj = 0.0, gr = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (64 * j < N) {
                const double r = amp * g[j] - q[j] * d[j], jb = amp * g[j] * lx[j];
                rr += r * r; jr += jb * r; jj += jb * jb; gj += g[j] * jb; gr += g[j] * r;
            }
        rr = wave_sum(rr); jr = wave_sum(jr); jj = wave_sum(jj); gj = wave_sum(gj); gr = wave_sum(gr);
        cost = 0.5 * rr;
        const double num = clipped ? jr : jr - gj * gr / gg, den = clipped ? jj : jj - gj * gj / gg;
        ok = (gg > 0.0 && den > 0.0 && finite_d(num) && finite_d(den) && finite_d(rr)) ? 1 : 0;
        step = ok ? -num / den : 0.0;
    }
};

template <typename T, int CPL>
__global__ __launch_bounds__(64 * FB_LOSFIT_ROWS) void k_los_powerlaw(const PlawArgs a) {
    const int lane = threadIdx.x & 63, N = a.N;
    const long long p = (long long)blockIdx.x * FB_LOSFIT_ROWS + (threadIdx.x >> 6);
    if (p >= a.npix) return;                                   // wave-uniform; the kernel has no barrier
    const T* row = (const T*)a.maps + p * N;
    PlawRow<CPL> R;
    R.N = N;
    unsigned goodmask = 0;
    int nonfinite = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < N;
        const double wv = in ? aux_at<T>(a.w, a.w_kind, p * N + c, c) : 0.0;
        const bool good = in && wv != 0.0;
        const double t = in ? (double)row[c] - (a.tpsmean ? a.tpsmean[c] : 0.0) : 0.0;
        R.d[j] = good ? t : 0.0;
        R.q[j] = good ? wv / aux_at<T>(a.sigma, a.s_kind, p * N + c, c) : 0.0;
        R.lx[j] = in ? a.lnx[c] : 0.0;
        R.g[j] = 0.0;
        if (good) goodmask |= 1u << j;
        nonfinite |= __any(good && !finite_d(t));
    }
    // the first and the fourth unflagged channel
    int cprev = -1, cfirst = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int m = 0x7fffffff;
#pragma unroll
        for (int j = CPL - 1; j >= 0; --j) {
            const int c = lane + 64 * j;
            if (((goodmask >> j) & 1u) && c > cprev) m = c;
        }
        m = wave_minmax<false>(m);
        if (r == 0) cfirst = m;
        cprev = m;
    }
    const int cfourth = cprev;
    int status = cfourth == 0x7fffffff ? FB_LOSFIT_TOO_FEW : (nonfinite ? FB_LOSFIT_NONFINITE : FB_LOSFIT_OK);
    double d0 = 0.0, d3 = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        d0 += c == cfirst ? R.d[j] : 0.0;
        d3 += c == cfourth ? R.d[j] : 0.0;
    }
    d0 = wave_sum(d0); d3 = wave_sum(d3);                     // one term and zeros: exact
    double b = 0.0;
    if (status == FB_LOSFIT_OK) {
        if (a.beta_guess) b = a.beta_guess[p];
        else b = log(d3 / d0) / (a.lnx[cfourth] - a.lnx[cfirst]);
        if (!(d0 > 0.0) || (!a.beta_guess && !(d3 / d0 > 0.0)) || !finite_d(b)) status = FB_LOSFIT_NONPOSITIVE;
    }
    status = uniform(status);
    double beta = b, amp = 0.0, cost = 0.0, syamp = 0.0, ffamp = 0.0;
    int it = 0;
    if (status == FB_LOSFIT_OK) {
        const double blo = fmin(0.9 * b, 1.1 * b), bhi = fmax(0.9 * b, 1.1 * b);
        R.alo = 0.5 * d0; R.ahi = 1.5 * d0;
        double step;
        int ok, converged = 0;
        R.eval(beta, amp, cost, step, ok);
        if (!uniform(ok)) status = FB_LOSFIT_SINGULAR;
        for (; status == FB_LOSFIT_OK && !converged && it < a.max_iter; ++it) {
            // the step, clipped to the interval of beta, halved while the cost rises (at most max_iter times)
            double bn = fmin(fmax(beta + step, blo), bhi), ampn = amp, costn = cost, stepn = 0.0;
            int moved = 0;
            for (int h = 0; h <= a.max_iter; ++h) {
                if (uniform(fabs(bn - beta) <= a.tol * fmax(1.0, fabs(beta)))) break;
                R.eval(bn, ampn, costn, stepn, ok);
                if (!uniform(ok)) { status = FB_LOSFIT_SINGULAR; break; }
                if (uniform(costn <= cost)) { moved = 1; break; }
                step *= 0.5;
                bn = fmin(fmax(beta + step, blo), bhi);
            }
            if (status != FB_LOSFIT_OK) break;
            if (moved) { beta = bn; amp = ampn; cost = costn; step = stepn; }
            else converged = 1;                                  // no step above the tolerance lowers the cost
        }
        if (status == FB_LOSFIT_OK && !converged) status = FB_LOSFIT_MAXITER;
    }
    // the two-template solve on the unflagged channels, unweighted: S = [x^betaS, x^freeind]
    if (status == FB_LOSFIT_OK) {
        double s11 = 0.0, s12 = 0.0, s22 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (((goodmask >> j) & 1u)) {
                const double e1 = exp(beta * R.lx[j]), e2 = exp(a.freeind * R.lx[j]);
                s11 += e1 * e1; s12 += e1 * e2; s22 += e2 * e2; t1 += e1 * R.d[j]; t2 += e2 * R.d[j];
            }
        s11 = wave_sum(s11); s12 = wave_sum(s12); s22 = wave_sum(s22); t1 = wave_sum(t1); t2 = wave_sum(t2);
        const double det = s11 * s22 - s12 * s12;
        // singular to working precision: 1 - cos^2 of the angle between the templates below 1e-14
        if (!uniform(det > 1e-14 * s11 * s22 && finite_d(det) && finite_d(t1) && finite_d(t2))) status = FB_LOSFIT_SINGULAR;
        else { syamp = (s22 * t1 - s12 * t2) / det; ffamp = (s11 * t2 - s12 * t1) / det; }
    }
    T* orow = (T*)a.resid + p * N;
    T* mrow = a.model ? (T*)a.model + p * N : nullptr;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        if (c < N) {
            if (status != FB_LOSFIT_OK) {
                orow[c] = (T)NAN;
                if (mrow) mrow[c] = (T)NAN;
            } else {
                const double m = syamp * exp(beta * R.lx[j]) + ffamp * exp(a.freeind * R.lx[j]);
                orow[c] = ((goodmask >> j) & 1u) ? (T)(R.d[j] - m) : (T)0;
                if (mrow) mrow[c] = (T)m;
            }
        }
    }
    if (lane == 0) {
        const bool fine = status == FB_LOSFIT_OK;
        a.rows[p] = fine ? beta : NAN;
        a.rows[a.npix + p] = fine ? amp : NAN;
        a.rows[2 * a.npix + p] = fine ? syamp : NAN;
        a.rows[3 * a.npix + p] = fine ? ffamp : NAN;
        a.rows[4 * a.npix + p] = fine ? cost : NAN;
        a.n_iter[p] = it;
        a.status[p] = status;
        if (!fine) atomicAdd(a.n_failed, 1);
    }
}

// ---- the finish of the Gaussian-process filter: out = X - Y - shift[c], stored in the plan's precision --------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_los_subtract(const T* __restrict__ X, const double* __restrict__ Y,
                                                      const double* __restrict__ shift, T* __restrict__ out, long long n, int N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (T)(((double)X[i] - shift[i % N]) - Y[i]);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
// channels per lane: 1 up to 64 channels, 4 up to 256, 16 up to 1024
template <typename T, typename Args, typename F1, typename F4, typename F16>
int launch_rows(fb_plan* p, const Args& a, F1 k1, F4 k4, F16 k16, const char* name, hipStream_t s) {
    const dim3 grid((unsigned)((a.npix + FB_LOSFIT_ROWS - 1) / FB_LOSFIT_ROWS)), block(64 * FB_LOSFIT_ROWS);
    FbProfScope _ps(p, FBK_PCA, s);
    if (a.N <= 64) hipLaunchKernelGGL(k1, grid, block, 0, s, a);
    else if (a.N <= 256) hipLaunchKernelGGL(k4, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k16, grid, block, 0, s, a);
    FB_LAUNCH_CHECK(name);
    return FB_OK;
}
template <typename T>
int polyfit(fb_plan* p, const PolyArgs& a, hipStream_t s) {
    return launch_rows<T>(p, a, k_los_polyfit<T, 1>, k_los_polyfit<T, 4>, k_los_polyfit<T, 16>, "k_los_polyfit", s);
}
template <typename T>
int powerlaw(fb_plan* p, const PlawArgs& a, hipStream_t s) {
    return launch_rows<T>(p, a, k_los_powerlaw<T, 1>, k_los_powerlaw<T, 4>, k_los_powerlaw<T, 16>, "k_los_powerlaw", s);
}
template <typename T>
int subtract(fb_plan* p, const void* X, const double* Y, const double* shift, void* out, hipStream_t s) {
    const long long n = (long long)p->N * p->N * p->N;
    FbProfScope _ps(p, FBK_REALOP, s);
    hipLaunchKernelGGL((k_los_subtract<T>), dim3(grid_for((unsigned long long)n, p)), dim3(256), 0, s, (const T*)X, Y, shift, (T*)out, n, p->N);
    FB_LAUNCH_CHECK("k_los_subtract");
    return FB_OK;
}

// the counter of failed rows lives at the start of the plan's shared work buffer; the entry points read it back before they return
int failed_begin(fb_plan* p, int** counter, hipStream_t s) {
    FB_TRY(p->work.ensure(sizeof(int)));
    *counter = p->work.as<int>();
    FB_HIP(hipMemsetAsync(*counter, 0, sizeof(int), s));
    return FB_OK;
}
bool kind_ok(const void* a, int kind) { return !a || kind == FB_GCR_PER_CHANNEL || kind == FB_GCR_PER_VOXEL; }

}  // namespace

extern "C" {

int fb_los_polyfit(fb_plan* p, const void* cube, const void* w, int w_kind, const double* basis_dev, const double* pinv_dev, int order,
                   int log_y, void* cube_out, void* model_out, double* coeffs_dev, double* chi2_dev, int32_t* status_dev,
                   int32_t* n_failed_out, void* stream) {
    FB_REQUIRE(p && cube && basis_dev && cube_out && status_dev && n_failed_out, "null pointer");
    FB_REQUIRE(order >= 0 && order < FB_LOSFIT_KMAX, "fb_los_polyfit: order 0 .. 7");
    FB_REQUIRE(kind_ok(w, w_kind), "w_kind: FB_GCR_PER_CHANNEL or FB_GCR_PER_VOXEL");
    FB_REQUIRE(!pinv_dev || !w || w_kind == FB_GCR_PER_CHANNEL, "fb_los_polyfit: a shared pseudo-inverse goes with no or per-channel weights");
    FB_REQUIRE(p->N <= FB_LOSFIT_NMAX, "fb_los_polyfit: at most 1024 channels");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    PolyArgs a;
    a.cube = cube; a.w = w; a.w_kind = w_kind; a.basis = basis_dev; a.pinv = pinv_dev; a.K1 = order + 1; a.logy = log_y ? 1 : 0;
    a.out = cube_out; a.model = model_out; a.coeffs = coeffs_dev; a.chi2 = chi2_dev; a.status = status_dev;
    a.npix = (long long)p->N * p->N; a.N = p->N;
    int r = failed_begin(p, &a.n_failed, s);
    if (r) return r;
    r = FB_DISPATCH(p, polyfit<float>(p, a, s), polyfit<double>(p, a, s));
    if (r) return r;
    return fb_read_back(n_failed_out, a.n_failed, sizeof(int32_t), s);
}

int fb_los_powerlaw(fb_plan* p, const void* maps, const double* tpsmean_dev, const void* sigma, int sigma_kind, const void* w,
                    int w_kind, const double* lnx_dev, double freeind, const double* beta_guess_dev, int max_iter, double tol,
                    void* resid_out, void* model_out, double* rows_dev, int32_t* n_iter_dev, int32_t* status_dev,
                    int32_t* n_failed_out, void* stream) {
    FB_REQUIRE(p && maps && lnx_dev && resid_out && rows_dev && n_iter_dev && status_dev && n_failed_out, "null pointer");
    FB_REQUIRE(kind_ok(w, w_kind) && kind_ok(sigma, sigma_kind), "w_kind, sigma_kind: FB_GCR_PER_CHANNEL or FB_GCR_PER_VOXEL");
    FB_REQUIRE(max_iter >= 1 && max_iter <= 100000 && tol > 0.0, "fb_los_powerlaw: 1 <= max_iter <= 100000 and tol > 0");
    FB_REQUIRE(p->N <= FB_LOSFIT_NMAX, "fb_los_powerlaw: at most 1024 channels");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    PlawArgs a;
    a.maps = maps; a.tpsmean = tpsmean_dev; a.sigma = sigma; a.s_kind = sigma_kind; a.w = w; a.w_kind = w_kind; a.lnx = lnx_dev;
    a.freeind = freeind; a.beta_guess = beta_guess_dev; a.max_iter = max_iter; a.tol = tol; a.resid = resid_out; a.model = model_out;
    a.rows = rows_dev; a.n_iter = n_iter_dev; a.status = status_dev; a.npix = (long long)p->N * p->N; a.N = p->N;
    int r = failed_begin(p, &a.n_failed, s);
    if (r) return r;
    r = FB_DISPATCH(p, powerlaw<float>(p, a, s), powerlaw<double>(p, a, s));
    if (r) return r;
    return fb_read_back(n_failed_out, a.n_failed, sizeof(int32_t), s);
}

int fb_los_subtract(fb_plan* p, const void* X, const double* Y, const double* shift_dev, void* cube_out, void* stream) {
    FB_REQUIRE(p && X && Y && shift_dev && cube_out, "null pointer");
    FB_REQUIRE(cube_out != X && cube_out != (const void*)Y, "fb_los_subtract: cube_out must not be X or Y");
    FB_USE_DEVICE(p);
    hipStream_t s = (hipStream_t)stream;
    return FB_DISPATCH(p, subtract<float>(p, X, Y, shift_dev, cube_out, s), subtract<double>(p, X, Y, shift_dev, cube_out, s));
}

}  // extern "C"
