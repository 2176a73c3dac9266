"""Constructed inputs for the PCA primitives (fb_channel_means, fb_channel_covariance, fb_pca_clean, fb_rotated_covariance,
fb_nndsvd_norms, fb_nndsvd_fill) with expectations that hold bit for bit.

Every value is a small integer or a multiple of a small power of two, so every product and every sum the kernels form -- in
any order, fused or not, in fp64, and in fp32 where a result is stored in fp32 -- is exact: a correct device result EQUALS the
numpy one (BLAS included), and a comparison needs no tolerance.  Only the two final scalings round, and they are written here
as the header defines them: sums * (1.0 / npix) and S * (1.0 / (npix - 1)).  tests/test_pca_cases_cpu.py checks these
expectations against independent statements and checks that every intermediate stays in the exact range."""
import ctypes
import functools

import numpy as np

NUM_CU = (1, 8, 64, 104, 228, 256, 304)


def supported_sizes():
    """Even grid sizes 16 .. 1024 with no prime factor beyond 5."""
    out = []
    for n in range(16, 1025, 2):
        m = n
        for f in (2, 3, 5):
            while m % f == 0:
                m //= f
        if m == 1:
            out.append(n)
    return out


def plan(N, num_cu):
    """(slices, rows per slice) of fb_channel_covariance, from the library (host only)."""
    from fastbox_amd import _lib
    slices, rows = ctypes.c_int(-1), ctypes.c_int64(-1)
    _lib.call("fb_channel_covariance_plan", int(N), int(num_cu), ctypes.byref(slices), ctypes.byref(rows))
    return slices.value, rows.value


# ---- cubes: (npix, N) matrices, the pixel first as the device holds them ---------------------------------------------------
def channel_offsets(N):
    """The integer mean of every channel of int_cube: -2 .. 2."""
    return (np.arange(N) * 3) % 5 - 2


@functools.lru_cache(maxsize=2)
def int_cube(N):
    """int8 (N^2, N): integers in [-8, 8], fixed seed.  Pixel npix - 1 - p holds minus the draw of pixel p, so the draws of
    every channel sum to zero and channel c has the integer mean channel_offsets(N)[c] (npix is even)."""
    npix = N * N
    rs = np.random.RandomState(1000 + N)
    x = np.empty((npix, N), dtype=np.int8)
    half = rs.randint(-6, 7, size=(npix // 2, N)).astype(np.int8)
    x[:npix // 2] = half
    x[npix // 2:] = -half[::-1]
    x += channel_offsets(N).astype(np.int8)
    x.setflags(write=False)
    return x


def hot_spectrum(N):
    """The integer spectrum of the one hot pixel: every channel non-zero, not symmetric about the middle."""
    v = (np.arange(N) * 7 + 3) % 17 - 8
    v[v == 0] = 5
    return v.astype(np.float64)


def one_hot(N, p):
    x = np.zeros((N * N, N))
    x[p] = hot_spectrum(N)
    return x


def hot_positions(N, slices, rows):
    """Pixels at which k_channel_cov can go wrong, by name: the ends, both sides of the first slice boundary, every p mod 4, rows
    beyond slice 0 that its last pipeline group (16 rows) fetches and masks, the first row of the last slice's last group."""
    npix = N * N
    pos = {"first": 0, "last": npix - 1}
    mid = (npix // 2) & ~3
    for r in range(4):
        pos["mod4=%d" % r] = mid + r
    if slices > 1:
        pos["end of slice 0"] = rows - 1
        pos["start of slice 1"] = rows
        for d in (1, 6, 11):
            if rows % 16 and d < 16 - rows % 16 and rows + d < npix:
                pos["masked tail of slice 0 +%d" % d] = rows + d
    last0 = (slices - 1) * rows
    pos["last group of the last slice"] = last0 + ((npix - 1 - last0) // 16) * 16
    return pos


# ---- means -----------------------------------------------------------------------------------------------------------------
def expected_means(x):
    npix = x.shape[0]
    return x.sum(axis=0, dtype=np.int64).astype(np.float64) * (1.0 / npix)


def quarter_means(N):
    return ((np.arange(N) * 3) % 13 - 6) * 0.25


def mean_vectors(N, x=None):
    out = {"zeros": np.zeros(N), "quarters": quarter_means(N)}
    if x is not None:
        out["own"] = expected_means(x)
    return out


# ---- covariance ------------------------------------------------------------------------------------------------------------
def expected_cov(x, mean):
    """np.cov's divisor, about `mean` whatever it is: S * (1.0 / (npix - 1)), S = sum_p (x_p - mean)(x_p - mean)^T."""
    npix = x.shape[0]
    d = x.astype(np.float64) - mean
    return (d.T @ d) * (1.0 / (npix - 1))


def expected_cov_one_hot(N, mean):
    """The same for one_hot(N, p), any p: npix - 1 pixels of -mean and one of v - mean."""
    npix = N * N
    d = hot_spectrum(N) - mean
    return ((npix - 1) * np.outer(mean, mean) + np.outer(d, d)) * (1.0 / (npix - 1))


# ---- projection ------------------------------------------------------------------------------------------------------------
def modes(N, nm):
    """U[N][nm]: column m has at most four non-zeros, +-2^-k with k = m mod 3; NOT orthonormal (out = x - U (U^T x) holds for
    any U).  Column 0 is never empty, neighbouring columns overlap, the last channel is used."""
    U = np.zeros((N, max(nm, 1)))
    for m in range(nm):
        rows = [(5 * m + 1) % N, (7 * m + 3) % N, (N - 1 - 3 * m) % N, (11 * m + N // 2) % N]
        for i, c in enumerate(rows):
            U[c, m] = (-1.) ** (i + m) * 2. ** -(m % 3)         # a repeated row keeps the last sign: still at most four
    return np.ascontiguousarray(U[:, :nm])


def expected_clean(x, mean, U, out_dtype=np.float64, chunk=1 << 16):
    """(cleaned (npix, N) in out_dtype, amps (nm, npix)): x - mean - U U^T (x - mean) per pixel."""
    npix, N = x.shape
    nm = U.shape[1]
    out = np.empty((npix, N), dtype=out_dtype)
    amps = np.empty((nm, npix))
    for a in range(0, npix, chunk):
        d = x[a:a + chunk].astype(np.float64) - mean
        A = d @ U
        full = d - A @ U.T
        out[a:a + chunk] = full
        assert np.array_equal(out[a:a + chunk], full), "the cleaned values leave the exact range of the stored type"
        amps[:, a:a + chunk] = A.T
    return out, amps


# ---- rotation --------------------------------------------------------------------------------------------------------------
def rotation(N):
    """Vt[N][N]: row m has at most four non-zeros in {-1, 1}; not symmetric (row m reaches channels m, m + 1, 3 m + 2, N - 1 - m
    only), so that a transposed read gives another matrix."""
    Vt = np.zeros((N, N))
    for m in range(N):
        for i, c in enumerate((m, (m + 1) % N, (3 * m + 2) % N, N - 1 - m)):
            Vt[m, c] = (-1.) ** (i * (m + 1))
    assert not np.array_equal(Vt, Vt.T)
    return Vt


def expected_rotated(x, Vt):
    """(B^T B) * (1.0 / (npix - 1)), B = X Vt^T, not centred."""
    npix = x.shape[0]
    B = x.astype(np.float64) @ Vt.T
    return (B.T @ B) * (1.0 / (npix - 1))


# ---- NNDSVD rows -----------------------------------------------------------------------------------------------------------
EPS = 0.25


def nndsvd_rows(k, npix):
    """W[k][npix]: signed quarter-integers in [-4, 4], zeros included."""
    rs = np.random.RandomState(77 + k + npix)
    return rs.randint(-16, 17, size=(k, npix)) * 0.25


def expected_norms(W):
    out = np.empty(2 * W.shape[0])
    out[0::2] = np.sum(np.where(W > 0., W, 0.) ** 2, axis=1)
    out[1::2] = np.sum(np.where(W > 0., 0., W) ** 2, axis=1)
    return out


def nndsvd_coef(k):
    """Powers of two of both signs: coef[j] * w is exact."""
    return np.array([(-1.) ** (j // 2) * 2. ** ((j % 3) - 1) for j in range(k)])


def nndsvd_fill_rows(k, npix):
    """nndsvd_rows with, in every row, values that land exactly on EPS and on the double just below it after the scaling."""
    W = nndsvd_rows(k, npix)
    coef = nndsvd_coef(k)
    below = np.nextafter(EPS, 0.)
    for j in range(k):
        W[j, 3 + j] = EPS / coef[j]
        W[j, 40 + 2 * j] = below / coef[j]
        W[j, npix - 1 - j] = -EPS / coef[j]
    return W


def expected_fill(W, coef, abs_first, eps, fill):
    v = coef[:, None] * W
    out = np.maximum(v, 0.)
    if abs_first:
        out[0] = np.abs(v[0])
    return np.where(out < eps, fill, out)


# ---- the sizes of tests/test_pca_kernels_gpu.py, by kernel instance -----------------------------------------------------------
COV_SIZES = {"MA=1": (16, 48, 80), "MA=1 edge": (18, 24, 30), "MA=1 edge, once empty slices": (50, 60, 90),
             "MA=2": (32, 96, 160), "MA=4": (64, 128, 320)}
F32_ONLY = (320, 512)                                  # sizes run in single precision only
CLEAN_SIZES = {1: (16, 18, 64), 2: (80, 128), 4: (160, 250, 256), 8: (384, 512)}      # channels per lane -> N
CLEAN_PREC = {384: ("f64",), 512: ("f32",)}
ROTATED_SIZES = (16, 18, 50, 64, 96, 128, 160, 256, 384)
ROTATED_PREC = {384: ("f32",)}
NNDSVD_SIZES = (16, 18, 64)
