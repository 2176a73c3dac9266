"""CPU: the constructed PCA cases (tests/pca_cases.py) against independent statements, the exact range of every intermediate,
and the pixel-slice plan of fb_channel_covariance -- the regression test of its former read past the cube."""
import numpy as np
import pytest

from tests import pca_cases as pc

ALL_COV = sorted(n for v in pc.COV_SIZES.values() for n in v)


def _ld_cov(x, mean):
    """Per-pixel loop in extended precision: sum of outer products about `mean`, then np.cov's divisor."""
    npix, N = x.shape
    S = np.zeros((N, N), dtype=np.longdouble)
    m = mean.astype(np.longdouble)
    for p in range(npix):
        d = x[p].astype(np.longdouble) - m
        S += np.outer(d, d)
    return S, (S / np.longdouble(npix - 1)).astype(np.float64)


@pytest.mark.parametrize("N", [16, 18])
def test_expectations_agree_with_independent_statements(N):
    x = pc.int_cube(N)
    npix = N * N
    own = pc.expected_means(x)
    assert np.array_equal(own, pc.channel_offsets(N).astype(np.float64))
    assert np.array_equal(own, np.mean(x.astype(np.float64), axis=0))
    for name, mean in pc.mean_vectors(N, x).items():
        want = pc.expected_cov(x, mean)
        S, ld = _ld_cov(x, mean)
        # S is exact in both, so the two differ by the rounding of S * (1 / (npix - 1)) against S / (npix - 1): 2 ulp at most
        assert np.all(np.abs(want - ld) <= 2 * np.spacing(np.abs(ld))), name
        d = x.astype(np.float64) - mean
        assert np.array_equal(d.T @ d, S.astype(np.float64)), name                  # BLAS forms the exact sums
    c = np.cov(x.astype(np.float64).T)
    want = pc.expected_cov(x, own)
    assert np.max(np.abs(c - want)) <= 4 * np.finfo(float).eps * np.max(np.abs(want))
    # one hot pixel: the closed form against the dense one and, about zero, against v v^T
    v = pc.hot_spectrum(N)
    for p in pc.hot_positions(N, *pc.plan(N, 256)).values():
        for name, mean in pc.mean_vectors(N).items():
            assert np.array_equal(pc.expected_cov_one_hot(N, mean), pc.expected_cov(pc.one_hot(N, p), mean)), (p, name)
    assert np.array_equal(pc.expected_cov_one_hot(N, np.zeros(N)), np.outer(v, v) * (1.0 / (npix - 1)))
    # projection and rotation, pixel by pixel in extended precision
    for nm in (0, 1, 3, 8, N):
        U = pc.modes(N, nm)
        assert U.shape == (N, nm) and np.all(np.count_nonzero(U, axis=0) <= 4) and (nm == 0 or np.any(U[:, 0]))
        for name, mean in pc.mean_vectors(N, x).items():
            out, amps = pc.expected_clean(x, mean, U)
            Ul = U.astype(np.longdouble)
            for p in range(0, npix, 7):
                d = x[p].astype(np.longdouble) - mean.astype(np.longdouble)
                a = Ul.T @ d
                assert np.array_equal(amps[:, p], a.astype(np.float64)) and np.array_equal(out[p], (d - Ul @ a).astype(np.float64))
    Vt = pc.rotation(N)
    assert np.all(np.count_nonzero(Vt, axis=1) <= 4) and set(np.unique(Vt)) <= {-1., 0., 1.}
    B = np.array([[sum(Vt[m, c] * float(x[p, c]) for c in range(N)) for m in range(N)] for p in range(npix)])
    S = np.zeros((N, N))
    for p in range(npix):
        S += np.outer(B[p], B[p])
    assert np.array_equal(pc.expected_rotated(x, Vt), S * (1.0 / (npix - 1)))
    assert not np.array_equal(pc.expected_rotated(x, Vt), pc.expected_rotated(x, Vt.T))


def _dyadic(a, frac_bits):
    """Every entry of a is a multiple of 2^-frac_bits."""
    s = np.asarray(a, dtype=np.float64) * 2. ** frac_bits
    return bool(np.all(s == np.rint(s)))


@pytest.mark.parametrize("N", sorted(set(ALL_COV) | set(pc.ROTATED_SIZES) | {n for v in pc.CLEAN_SIZES.values() for n in v}))
def test_every_intermediate_stays_in_the_exact_range(N):
    """Bounds from the constructions alone (no big products): a sum whose terms are multiples of 2^-f and whose absolute values add
    up to less than 2^(53 - f) is exact in fp64 in any order; a stored value with fewer than 24 significant bits is exact in fp32."""
    npix = N * N
    off = pc.channel_offsets(N).astype(np.float64)
    # the means: integer sums, |sum| <= 8 npix, and the cube's own mean is the exact integer offset
    assert 8 * npix < 2 ** 24
    assert np.array_equal((off * npix) * (1.0 / npix), off), "sums * (1.0 / npix) must be the exact integer mean"
    worst = 0.
    for mean in (off, np.zeros(N), pc.quarter_means(N)):
        assert _dyadic(mean, 2)
        worst = max(worst, 8. + np.max(np.abs(mean)))               # |x - mean|, a multiple of 1/4
    hot = np.max(np.abs(pc.hot_spectrum(N))) + np.max(np.abs(pc.quarter_means(N)))
    worst = max(worst, hot)
    # covariance: terms multiples of 1/16
    assert npix * worst * worst * 16 < 2 ** 53
    # projection: U = +-2^-k, k <= 2, at most 4 per column: amps multiples of 2^-4 below 4 worst; rec multiples of 2^-6, at
    # most nm terms below 4 worst each
    for nm in (1, 3, 8) + ((N,) if N <= 18 else ()):
        U = pc.modes(N, nm)
        assert _dyadic(U, 2) and np.max(np.abs(U)) <= 1. and np.all(np.count_nonzero(U, axis=0) <= 4)
        per_row = np.max(np.sum(np.abs(U), axis=1))                # sum_m |U[c][m]|
        biggest = worst + per_row * 4 * worst                      # |x - rec|
        assert biggest * 2 ** 6 < 2 ** 24, "cleaned values must fit fp32 exactly"
    # rotation: B integers below 4 * 8, B^T B below npix 32^2
    assert npix * 32 * 32 < 2 ** 53
    # NNDSVD rows: squares of quarter-integers up to 4 (and scaled by a power of two in the fill)
    assert npix * 16 * 16 < 2 ** 53


@pytest.mark.parametrize("k", [1, 5, 16])
def test_nndsvd_expectations(k):
    npix = 18 * 18
    W = pc.nndsvd_rows(k, npix)
    assert _dyadic(W, 2) and np.any(W == 0.) and np.any(W > 0.) and np.any(W < 0.)
    want = pc.expected_norms(W)
    for j in range(k):
        sp = sum(float(v) ** 2 for v in W[j] if v > 0.)
        sn = sum(float(v) ** 2 for v in W[j] if not v > 0.)
        assert want[2 * j] == sp and want[2 * j + 1] == sn
    coef = pc.nndsvd_coef(k)
    assert np.all(np.abs(coef) == 2. ** np.round(np.log2(np.abs(coef)))) and (k < 3 or np.any(coef < 0.))
    W2 = pc.nndsvd_fill_rows(k, npix)
    fill = -3.5                                                     # a value the rectified rows cannot hold otherwise
    for abs_first in (0, 1):
        got = pc.expected_fill(W2, coef, abs_first, pc.EPS, fill)
        for j in range(k):
            for p in range(npix):
                v = coef[j] * W2[j, p]
                v = abs(v) if (j == 0 and abs_first) else max(v, 0.)
                assert got[j, p] == (fill if v < pc.EPS else v)
        # the two edges: exactly eps is kept, the double below it is filled
        for j in range(k):
            if coef[j] > 0.:
                assert got[j, 3 + j] == pc.EPS and got[j, 40 + 2 * j] == fill
        assert got[0, npix - 1] == (pc.EPS if abs_first else fill)


# ---- the pixel-slice plan --------------------------------------------------------------------------------------------------
def _parent_slices(N, num_cu):
    """The launcher and kernel before the plan was made one function: the launcher chose the number of slices, the kernel derived
    the rows per slice from it and rounded them up to a multiple of four."""
    npix = N * N
    MA = 4 if N % 64 == 0 else (2 if N % 32 == 0 else 1)
    bs = 16 * MA
    nbs = (N + bs - 1) // bs
    npairs = nbs * (nbs + 1) // 2
    slices = (8 * num_cu + npairs - 1) // npairs
    slices = max(1, min(slices, npix // 64))
    per = ((npix + slices - 1) // slices + 3) & ~3
    return slices, per


def _empty(N, slices, rows):
    return [q for q in range(slices) if q * rows >= N * N]


def test_parent_formula_left_empty_slices_that_start_past_the_cube():
    bad = [N for N in pc.supported_sizes() if _empty(N, *_parent_slices(N, 256))]
    assert bad == [50, 54, 60, 90, 108]
    # such a slice fetched row p0 = q rows >= npix whole: the elements of the cube's type from the end of the cube to the farthest
    reach = {N: ((_parent_slices(N, 256)[0] - 1) * _parent_slices(N, 256)[1] - N * N) * N + N for N in bad}
    assert reach[50] == 4250 and reach[60] == 8460, reach
    for N in (16, 18, 32, 48, 80, 96, 256):
        assert not _empty(N, *_parent_slices(N, 256))              # why no earlier test could see it


@pytest.mark.parametrize("num_cu", pc.NUM_CU)
def test_plan_tiles_the_pixels_with_non_empty_slices(num_cu):
    for N in pc.supported_sizes():
        npix = N * N
        slices, rows = pc.plan(N, num_cu)
        assert slices >= 1 and rows >= 1, (N, slices, rows)
        assert not _empty(N, slices, rows), (N, slices, rows)                        # every slice is non-empty
        assert (slices - 1) * rows < npix <= slices * rows, (N, slices, rows)        # they tile [0, npix) exactly
        assert rows % 4 == 0 or slices == 1, (N, slices, rows)                       # all but the last: a multiple of 4 rows
        assert slices <= max(1, npix // 64), (N, slices, rows)
        # the rows per slice are the parent's, so every partial sum is the parent's: only the empty slices went
        pslices, prows = _parent_slices(N, num_cu)
        assert rows == prows and slices == pslices - len(_empty(N, pslices, prows)), (N, slices, rows)


def test_plan_rejects_bad_arguments():
    import ctypes
    from fastbox_amd import _lib
    lib = _lib.load()
    s, r = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.fb_channel_covariance_plan(16, 256, ctypes.byref(s), ctypes.byref(r)) == 0 and (s.value, r.value) == (4, 64)
    assert lib.fb_channel_covariance_plan(1, 256, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_channel_covariance_plan(16, 0, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_channel_covariance_plan(16, 256, None, ctypes.byref(r)) != 0
    assert lib.fb_channel_covariance_plan(16, 256, ctypes.byref(s), None) != 0
