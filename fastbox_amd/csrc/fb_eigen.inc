// Leading eigenvectors of the frequency-frequency covariance on the device (included at the end of fb_api.hip, inside extern "C").
//
// filters.py:161-169 takes np.linalg.eig of an N x N covariance (N = channels = the grid size), sorts by decreasing eigenvalue and
// keeps `nmodes` columns.  Here: cyclic two-sided Jacobi in fp64 with the round-robin ordering -- round r of a sweep rotates the
// N/2 disjoint index pairs of a tournament schedule at once, A <- J^T A J, V <- V J with J the product of the N/2 plane
// rotations that annihilate a_pq of their pair -- one launch per round over the (N/2)^2 2 x 2 blocks of A and the N x N/2 row
// pairs of V, double-buffered (every block reads the old matrix: its own four entries and the three entries that define each of
// its two rotations).  A sweep is N - 1 rounds; the off-diagonal norm falls quadratically once it is small, 6-10 sweeps in all.
// Jacobi's eigenvectors of a positive semi-definite matrix are accurate relative to each eigenvalue's own size (Demmel & Veselic
// 1992), which is what a foreground covariance spanning 10+ decades wants; the arithmetic is O(N^3) per sweep and nothing next
// to forming the covariance (N^4 / 2 multiply-adds on the fp64 matrix cores, k_channel_cov).
extern "C++" {
namespace {

// pair k (0 <= k < n/2) of round r (0 <= r < n-1) of the circle method on n players (n even): p < q
__device__ __forceinline__ void jacobi_pair(int n, int r, int k, int& p, int& q) {
    const int m = n - 1;
    int a, b;
    if (k == 0) { a = m; b = r; }
    else { a = r + k; if (a >= m) a -= m; b = r - k; if (b < 0) b += m; }
    p = a < b ? a : b; q = a < b ? b : a;
}
using fb::jacobi_rotation;           // fb_dev.h: the per-voxel 3 x 3 solver of fb_web.hip rotates with it too
// blockIdx.y < n/2: block row `a` of A; else: rows 2 j, 2 j + 1 of V, j = blockIdx.y - n/2.  Thread = pair b (columns).
__global__ __launch_bounds__(128) void k_jacobi_round(const double* __restrict__ A, double* __restrict__ An,
                                                      const double* __restrict__ V, double* __restrict__ Vn, int n, int r) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, half = n >> 1;
    if (b >= half) return;
    int pb, qb;
    jacobi_pair(n, r, b, pb, qb);
    double cb, sb;
    jacobi_rotation(A[(size_t)pb * n + pb], A[(size_t)qb * n + qb], A[(size_t)pb * n + qb], cb, sb);
    if ((int)blockIdx.y >= half) {
        const int i0 = 2 * ((int)blockIdx.y - half);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const size_t row = (size_t)(i0 + d) * n;
            const double vp = V[row + pb], vq = V[row + qb];
            Vn[row + pb] = vp * cb - vq * sb;
            Vn[row + qb] = vp * sb + vq * cb;
        }
        return;
    }
    const int a = blockIdx.y;
    // the block (a, b) with a > b is the transpose of the block (b, a): computed in that order, so that A stays symmetric
    // to the last bit
    const bool swap = a > b;
    int pa, qa;
    jacobi_pair(n, r, a, pa, qa);
    double ca, sa;
    jacobi_rotation(A[(size_t)pa * n + pa], A[(size_t)qa * n + qa], A[(size_t)pa * n + qa], ca, sa);
    const int pr = swap ? pb : pa, qr = swap ? qb : qa, pc = swap ? pa : pb, qc = swap ? qa : qb;     // rows, columns of the canonical block
    const double cr = swap ? cb : ca, sr = swap ? sb : sa, cc = swap ? ca : cb, sc = swap ? sa : sb;
    const double b00 = A[(size_t)pr * n + pc], b01 = A[(size_t)pr * n + qc], b10 = A[(size_t)qr * n + pc], b11 = A[(size_t)qr * n + qc];
    const double t00 = cr * b00 - sr * b10, t01 = cr * b01 - sr * b11, t10 = sr * b00 + cr * b10, t11 = sr * b01 + cr * b11;
    double n00 = t00 * cc - t01 * sc, n01 = t00 * sc + t01 * cc, n10 = t10 * cc - t11 * sc, n11 = t10 * sc + t11 * cc;
    if (a == b) { n01 = 0.0; n10 = 0.0; }                      // the annihilated pair
    if (!swap) {
        An[(size_t)pa * n + pb] = n00; An[(size_t)pa * n + qb] = n01; An[(size_t)qa * n + pb] = n10; An[(size_t)qa * n + qb] = n11;
    } else {
        An[(size_t)pa * n + pb] = n00; An[(size_t)pa * n + qb] = n10; An[(size_t)qa * n + pb] = n01; An[(size_t)qa * n + qb] = n11;
    }
}
// A = the symmetric part of C (a covariance is symmetric already: then A = C to the bit), V = 1
__global__ void k_eig_init(const double* __restrict__ C, double* __restrict__ A, double* __restrict__ V, int n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * n) return;
    const size_t r = i / n, c = i % n;
    A[i] = 0.5 * C[i] + 0.5 * C[c * n + r];
    V[i] = r == c ? 1.0 : 0.0;
}
// out[0] = sum of squares of the off-diagonal entries, out[1] = of all entries (one workgroup; fixed order)
__global__ __launch_bounds__(1024) void k_eig_norms(const double* __restrict__ A, int n, double* out) {
    __shared__ double so[1024], st[1024];
    double off = 0.0, tot = 0.0;
    for (size_t i = threadIdx.x; i < (size_t)n * n; i += 1024) {
        const double v = A[i], v2 = v * v;
        tot += v2;
        if (i / n != i % n) off += v2;
    }
    so[threadIdx.x] = off; st[threadIdx.x] = tot;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { so[threadIdx.x] += so[threadIdx.x + w]; st[threadIdx.x] += st[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = so[0]; out[1] = st[0]; }
}
// column i of V goes to column rank(i) of modes[n][nm] when its eigenvalue is among the nm largest (ties: lower index first)
__global__ __launch_bounds__(256) void k_eig_select(const double* __restrict__ A, const double* __restrict__ V, int n, int nm,
                                                    double* __restrict__ vals, double* __restrict__ modes) {
    __shared__ int cnt[256];
    const int i = blockIdx.x;
    const double di = A[(size_t)i * n + i];
    int c = 0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double dj = A[(size_t)j * n + j];
        c += (dj > di || (dj == di && j < i)) ? 1 : 0;
    }
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) cnt[threadIdx.x] += cnt[threadIdx.x + w]; __syncthreads(); }
    const int rank = cnt[0];
    if (rank >= nm) return;
    if (threadIdx.x == 0 && vals) vals[rank] = di;
    for (int row = threadIdx.x; row < n; row += 256) modes[(size_t)row * nm + rank] = V[(size_t)row * n + i];
}

}  // namespace
}  // extern "C++"

int fb_leading_eigenvectors(fb_plan* p, const double* cov_dev, int nmodes, double* modes_dev, double* vals_dev, int* sweeps_out,
                            void* stream) {
    FB_REQUIRE(p && cov_dev, "null pointer");
    FB_USE_DEVICE(p);
    const int n = p->N;
    FB_REQUIRE(nmodes >= 0 && nmodes <= n, "nmodes: 0 .. N");
    FB_REQUIRE(nmodes == 0 || modes_dev, "null pointer");
    if (sweeps_out) *sweeps_out = 0;
    if (nmodes == 0) return FB_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t nn = (size_t)n * n;
    FB_TRY(p->eig_work.ensure((4 * nn + 2) * sizeof(double)));      // not the shared work buffer: cov_dev may lie in it
    double* work = p->eig_work;
    double *A[2] = {work, work + nn}, *V[2] = {work + 2 * nn, work + 3 * nn}, *norms = work + 4 * nn;
    int cur = 0, sweeps = 0;
    double h[2] = {0.0, 0.0}, prev_off = -1.0;
    hipLaunchKernelGGL(k_eig_init, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, cov_dev, A[0], V[0], n);
    FB_LAUNCH_CHECK("k_eig_init");
    const dim3 grid((unsigned)((n / 2 + 127) / 128), (unsigned)n);
    for (;;) {
        hipLaunchKernelGGL(k_eig_norms, dim3(1), dim3(1024), 0, s, A[cur], n, norms);
        FB_LAUNCH_CHECK("k_eig_norms");
        FB_TRY(fb_read_back(h, norms, sizeof(h), s));
        if (!(h[1] == h[1]) || h[1] > 1.7e308) { fb_set_error("the matrix has non-finite entries"); return FB_ERR_INVALID; }
        if (h[0] <= 1e-30 * h[1]) break;                       // off-diagonal norm below 1e-15 of the matrix norm (or a zero matrix)
        // (at the rounding floor of a large matrix the norm stops falling: accept it there)
        if (prev_off >= 0.0 && h[0] <= 1e-26 * h[1] && h[0] > 0.25 * prev_off) break;
        prev_off = h[0];
        if (sweeps >= 60) { fb_set_error("Jacobi iteration did not converge in 60 sweeps"); return FB_ERR_STATE; }
        for (int r = 0; r < n - 1; ++r) {
            hipLaunchKernelGGL(k_jacobi_round, grid, dim3(128), 0, s, A[cur], A[cur ^ 1], V[cur], V[cur ^ 1], n, r);
            cur ^= 1;
        }
        FB_LAUNCH_CHECK("k_jacobi_round");
        ++sweeps;
        if (sweeps_out) *sweeps_out = sweeps;
    }
    hipLaunchKernelGGL(k_eig_select, dim3((unsigned)n), dim3(256), 0, s, A[cur], V[cur], n, nmodes, vals_dev, modes_dev);
    FB_LAUNCH_CHECK("k_eig_select");
    FB_HIP(hipStreamSynchronize(s));              // the caller reads sweeps_out and the outputs
    return FB_OK;
}
