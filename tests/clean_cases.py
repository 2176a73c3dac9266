"""Constructed inputs for the NMF and FastICA primitives (fb_nmf_sweep, fb_nmf_residual, fb_ica_step, fb_ica_sources, fb_real_min,
fb_complex_to_real) with expectations that hold bit for bit.

Every value is a small integer or a small dyadic fraction, so every product and every sum the kernels form -- in any order, fused
or not, in fp64, and in fp32 where a result is stored in fp32 -- is exact: a correct device result EQUALS the numpy one, and a
comparison needs no tolerance.  Only the documented final scaling sums * (1.0 / npix) rounds, and it is written here the same way.
The one exception is the H half of fb_nmf_sweep, which divides by entries of W^T W that are no powers of two: it is compared under
the rule of tests/test_cleaning_gpu.py with the difference of a float64 and a long double evaluation as delta_ref (h_half).
tests/test_clean_cases_cpu.py checks these expectations against independent statements and checks that every intermediate stays in
the exact range."""
import ctypes
import functools

import numpy as np

from tests import pca_cases as pc

KMAX = 16
FUN = {"logcosh": 0, "exp": 1, "cube": 2}                # FB_ICA_LOGCOSH, FB_ICA_EXP, FB_ICA_CUBE


def channels_per_lane(N):
    cpl = 1
    while 64 * cpl < N:
        cpl *= 2
    return cpl


# ---- the two pixel partitions, from the library (host only) -------------------------------------------------------------------
def sweep_plan(N, num_cu):
    """(workgroups, pixels per workgroup) of k_nmf_sweep."""
    from fastbox_amd import _lib
    nb, per = ctypes.c_int(-1), ctypes.c_int64(-1)
    _lib.call("fb_nmf_sweep_plan", int(N), int(num_cu), ctypes.byref(nb), ctypes.byref(per))
    return nb.value, per.value


def ica_plan(N):
    """(workgroups, pixels per workgroup) of k_ica_step."""
    from fastbox_amd import _lib
    nb, per = ctypes.c_int(-1), ctypes.c_int64(-1)
    _lib.call("fb_ica_step_plan", int(N), ctypes.byref(nb), ctypes.byref(per))
    return nb.value, per.value


def _named(pairs):
    """name -> pixel with distinct pixels: names that fall on one pixel are joined."""
    by_pixel = {}
    for name, p in pairs:
        by_pixel.setdefault(int(p), []).append(name)
    return {" / ".join(names): p for p, names in by_pixel.items()}


def sweep_positions(N, nb, per):
    """Pixels at which k_nmf_sweep can go wrong, by name: the ends, every p mod 4 (the wave that takes the pixel), both sides of the
    first workgroup boundary, the first and the last quad of the last non-empty workgroup (its last pixel is the cube's last)."""
    npix = N * N
    mid = ((npix // 2) & ~3) + 4
    last_wg = (npix - 1) // per
    pairs = [("first", 0), ("last = end of the last non-empty workgroup", npix - 1)]
    pairs += [("mod4=%d" % r, mid + r) for r in range(4)]
    if nb > 1 and per < npix:
        pairs += [("end of workgroup 0", per - 1), ("start of workgroup 1", per)]
    pairs += [("start of the last non-empty workgroup", last_wg * per), ("last quad of the last non-empty workgroup", (npix - 1) & ~3)]
    return _named(pairs)


def ica_positions(N, nb, per):
    """The same for k_ica_step (16 pixel lanes per row, steps of 16 pixels): also either side of the first step of workgroup 1, the
    first pixel of the last -- possibly ragged -- step of workgroup 0 and the start of the last non-empty workgroup."""
    npix = N * N
    mid = ((npix // 2) & ~3) + 4
    last_wg = (npix - 1) // per
    pairs = [("first", 0), ("last = end of the last non-empty workgroup", npix - 1)]
    pairs += [("mod4=%d" % r, mid + r) for r in range(4)]
    if nb > 1 and per < npix:
        pairs += [("end of workgroup 0 = end of its last step", per - 1), ("start of workgroup 1", per),
                  ("first pixel of the last step of workgroup 0", ((per - 1) // 16) * 16)]
        if per + 16 < npix:
            pairs += [("p0 + 15", per + 15), ("p0 + 16", per + 16)]
    pairs += [("start of the last non-empty workgroup", last_wg * per)]
    return _named(pairs)


# ---- cubes: (npix, N) matrices, the pixel first as the device holds them --------------------------------------------------------
XMAX = 16


def negated(npix):
    """The pixels whose spectrum is negated: with H >= 0 and a diagonal H H^T a non-negative cube can never clip a step."""
    return np.arange(npix) % 7 == 5


@functools.lru_cache(maxsize=2)
def nn_cube(N):
    """int8 (N^2, N): pca_cases.int_cube shifted to [0, 16], and every seventh pixel negated (see negated)."""
    x = pc.int_cube(N) + np.int8(8)
    x[negated(N * N)] *= np.int8(-1)
    x.setflags(write=False)
    return x


def hot_spectrum(N):
    """pca_cases.hot_spectrum made non-negative: integers in 1 .. 8, every channel non-zero."""
    return np.abs(pc.hot_spectrum(N))


# ---- NMF: the starts --------------------------------------------------------------------------------------------------------------
def w_start(k, npix):
    """W0[k][npix]: quarter-integers in [0, 4], a third of them zero."""
    rs = np.random.RandomState(31 + k + npix)
    W = rs.randint(0, 17, size=(k, npix)) * 0.25
    W[(np.arange(npix)[None, :] + np.arange(k)[:, None]) % 3 == 0] = 0.
    return W


def _row_values(n):
    """n values in {1, 2, 4} whose squares add up to a power of two (n is no multiple of 3: 2^e = n (mod 3) has a solution)."""
    assert n % 3
    e = 0
    while 2 ** e < n or (2 ** e - n) % 3:
        e += 1
    d = (2 ** e - n) // 3                                 # a + b + c = n, a + 4 b + 16 c = 2^e  =>  b + 5 c = d
    c = d // 10
    b = d - 5 * c
    a = n - b - c
    assert a >= 0 and a + 4 * b + 16 * c == 2 ** e
    return np.array([4.] * c + [2.] * b + [1.] * a)


def h_disjoint(N, k):
    """H0[k][N], rows with disjoint channel supports and entries in {0, 1, 2, 4}; every row's sum of squares is a power of two (or 0),
    so H H^T is diagonal and every step of the W half is exact.  Row 1 is all zero for k >= 2 (hess == 0).  Channel c belongs to
    the live row number (N - 1 - c) mod (live rows + 1) (k = 1: every channel to row 0), the last class to no row."""
    H = np.zeros((k, N))
    live = [t for t in range(k) if not (k >= 2 and t == 1)]
    classes = len(live) + (k > 1)
    owner = (N - 1 - np.arange(N)) % classes
    for j, t in enumerate(live):
        ch = np.flatnonzero(owner == j)
        if len(ch) % 3 == 0:
            ch = ch[1:]                                    # the last channels stay
        if len(ch):
            H[t, ch] = np.random.RandomState(N + 17 * k + t).permutation(_row_values(len(ch)))
    return H


def h_overlap(N, k):
    """H0[k][N] in {0, 1}: row t has ones at channels c_t and c_(t+1) of a chain 0 = c_0 < ... < c_k = N - 1, so H H^T has 2 on the
    diagonal and 1 beside it: every step halves once, W stays dyadic and gains one fraction bit per component."""
    assert 1 <= k <= 5
    c = [(j * (N - 1)) // k for j in range(k + 1)]
    H = np.zeros((k, N))
    for t in range(k):
        H[t, c[t]] = H[t, c[t + 1]] = 1.
    return H


H_START = {"disjoint": h_disjoint, "overlap": h_overlap}


# ---- NMF: one cyclic coordinate-descent pass, the definition of include/fastbox_hip.h -----------------------------------------------
def cd_pass(b, v0, A, dtype=np.float64, xp=np):
    """v[k][rows] from v0 with b[rows][k] (X H^T, or X^T W) and A[k][k] (H H^T, or W^T W).  Returns (v, violation).  xp: numpy, or
    torch for tensors on the device (fp64)."""
    k = len(A)
    v = v0.astype(dtype) if xp is np else v0.clone()
    viol = 0.
    for t in range(k):
        grad = -b[:, t]
        for r in range(k):
            grad = grad + A[t][r] * v[r]
        pg = xp.where(v[t] == 0, xp.clip(grad, None, 0.), grad)
        viol = viol + xp.abs(pg).sum()
        if A[t][t] != 0:
            v[t] = xp.clip(v[t] - grad / A[t][t], 0., None)
    return v, viol


def expected_w_half(XHt, W0, H0):
    """(W[k][npix], violation) after the W half: exact."""
    return cd_pass(XHt, W0, H0 @ H0.T)


def h_half(XtW, WtW, H0):
    """The H half on the exact X^T W [N][k] and W^T W: (H, violation, delta_ref of H relative to max|H|, delta_ref of the violation
    relative to itself) -- float64 against long double."""
    H, viol = cd_pass(XtW, H0, WtW)
    Hl, violl = cd_pass(XtW.astype(np.longdouble), H0, WtW.astype(np.longdouble), dtype=np.longdouble)
    scale = float(np.max(np.abs(Hl)))
    dref_h = float(np.max(np.abs(H - Hl))) / scale if scale else 0.
    dref_v = float(abs(viol - violl) / violl) if violl else 0.
    return H, float(viol), dref_h, dref_v


def one_hot_sums(N, p, W):
    """(X H^T is built by the caller) X^T W [N][k] of the cube that is zero but for hot_spectrum(N) at pixel p."""
    return np.outer(hot_spectrum(N), W[:, p])


# ---- NMF: the residual ------------------------------------------------------------------------------------------------------------
def residual_factors(N, k):
    """(W[k][npix], H[k][N]): integers in [-2, 2]."""
    rs = np.random.RandomState(500 + N + k)
    return rs.randint(-2, 3, size=(k, N * N)).astype(np.float64), rs.randint(-2, 3, size=(k, N)).astype(np.float64)


def expected_residual(x, W, H):
    """(X - W^T H as float64 (npix, N), its sum of squares)."""
    r = x - W.T @ H
    return r, float(np.sum(r * r))


# ---- FastICA ----------------------------------------------------------------------------------------------------------------------
def ica_inputs(n, npix):
    """(W[n][n] integers in [-2, 2] without a zero row, X1[n][npix] integers in [-4, 4])."""
    rs = np.random.RandomState(900 + n + npix % 1000)
    W = rs.randint(-2, 3, size=(n, n)).astype(np.float64)
    W[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2, -1., 2.)
    return W, rs.randint(-4, 5, size=(n, npix)).astype(np.float64)


def ica_hot_vector(W):
    """The integer n-vector of the one hot pixel of X1: every entry non-zero in [-4, 4], and no entry of W v zero."""
    n = len(W)
    for s in range(9):
        v = (np.arange(n) * 5 + 2 + s) % 9 - 4.
        v[v == 0] = 3.
        if np.all(W @ v != 0.):
            return v
    raise AssertionError("no hot vector for n = %d" % n)


def expected_ica_cube(W, X1):
    """(G[n][n], gp[n]) for g = y^3: (sum_p g(y) x^T) * (1.0 / npix), (sum_p 3 y^2) * (1.0 / npix)."""
    npix = X1.shape[1]
    y = W @ X1
    return ((y * y * y) @ X1.T) * (1.0 / npix), (3. * y * y).sum(axis=1) * (1.0 / npix)


def expected_ica_cube_one_hot(W, v, npix):
    y = W @ v
    return np.outer(y * y * y, v) * (1.0 / npix), (3. * y * y) * (1.0 / npix)


def real_ica_inputs(n, npix):
    """Real-valued (W, X1) for the two transcendental contrasts."""
    rs = np.random.RandomState(1300 + n)
    return rs.normal(size=(n, n)) / np.sqrt(n), rs.normal(size=(n, npix))


def source_scale(n):
    """Powers of two of both signs."""
    return np.array([(-1.) ** (i // 3) * 2. ** ((i % 4) - 2) for i in range(n)])


def expected_sources(W, scale, X1):
    """(S[n][npix], moments[2 n] = the means of S and of S^2, each sum * (1.0 / npix))."""
    npix = X1.shape[1]
    S = (W @ X1) * scale[:, None]
    return S, np.concatenate([S.sum(axis=1), (S * S).sum(axis=1)]) * (1.0 / npix)


# ---- fb_real_min and fb_complex_to_real ---------------------------------------------------------------------------------------------
RED_BLOCKS = 1024


def min_base(n, dtype):
    """Positive integers 3 .. 1002 in the cube's type."""
    return ((np.arange(n, dtype=np.int64) * 7) % 1000 + 3).astype(dtype)


def min_positions(n):
    """Elements at which the grid-stride reduction can go wrong, by name (256 threads per workgroup, at most 1024 workgroups)."""
    nb = min((n + 255) // 256, RED_BLOCKS)
    stride = nb * 256
    pairs = [("first", 0), ("last", n - 1), ("end of workgroup 0", 255), ("start of workgroup 1", 256), ("lane 63", 63),
             ("wave 1", 64)]
    if n > stride:
        pairs += [("end of the first stride", stride - 1), ("start of the second stride", stride),
                  ("start of the tail", (n // stride) * stride), ("in the tail", (n // stride) * stride + (n % stride) // 2)]
    else:
        pairs += [("start of the last workgroup", (nb - 1) * 256)]
    return _named(pairs)


def distinct_reals(n, dtype):
    """n distinct finite values of dtype: float32 by consecutive bit patterns from 1.0 (n may exceed 2^24), float64 the integers."""
    if np.dtype(dtype) == np.float32:
        return (np.arange(n, dtype=np.uint32) + np.uint32(0x3f800000)).view(np.float32)
    return np.arange(n, dtype=np.float64)


# ---- the sizes of tests/test_clean_kernels_gpu.py, by kernel instance ---------------------------------------------------------------
SWEEP_SIZES = {1: (16, 18, 64), 2: (72, 128), 4: (144, 256), 8: (270, 512), 16: (540, 1000)}      # channels per lane -> N
F32_ONLY = (512, 540, 1000)                             # sizes run in single precision only, their cubes built on the device
SWEEP_K = (1, 3, 16)
LARGEST_K = {1000: (3,)}                                # the sweep at N = 1000: k = 3 alone
OVERLAP_SIZES = (16, 18, 72)
OVERLAP_K = (2, 5)
RESIDUAL_K = (1, 5, 16)
HOT_SIZES = (16, 18, 64, 72, 128, 144, 270)             # one hot pixel: N <= 144 and N = 270
PLAIN_SIZES = (16, 18, 64, 72, 270)                     # the entries without a channels-per-lane instance
ICA_SIZES = PLAIN_SIZES + (512,)
ICA_N = (1, 2, 5, 16)
SOURCES_N = (1, 3, 16)
REAL_ICA_SIZES = (18, 270)
ALL_SIZES = tuple(sorted({n for v in SWEEP_SIZES.values() for n in v} | set(ICA_SIZES)))
