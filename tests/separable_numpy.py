"""Separable test fields and their exact transforms, in fp64, without an N^3 transform:

    x = sum_t a_t (x) b_t (x) c_t    =>    fftn(x) = sum_t fft(a_t) (x) fft(b_t) (x) fft(c_t)

A case is a list of terms (a, b, c) of real length-N vectors.  Every factor is an integer in [-127, 127] divided by 128 (8
significant bits), so a product of three has at most 24 and the field is held exactly by float32 storage: the reference is the
transform of what a single-precision device buffer actually contains.  Sums of terms stay exact where this module builds them:
the two-term case has its terms on disjoint x-planes (even / odd), the single mode is a sum of four products that are multiples
of 2^-21 below 4 in magnitude (24 bits).  A complex input takes its real part from one case and its imaginary part from another;
the transform is linear, so its reference is the same combination.

The spectrum is never formed as a whole on the host: `factor_spectra` gives the three transformed factor vectors per term,
`spectrum_plane` one x-plane of their outer product, `field_plane` one x-plane of the field.

Error bounds of a transform under test (`max_bound`, `rms_bound`), relative to the exact result `want`:
  max, random and two-term cases: the suite's convention (test_generic_grid_gpu.py), tol rms(want) sqrt(log2 N^3), tol = 3e-6
    (f32) / 1e-13 (f64);
  max, structured cases (impulses, Nyquist wave, single mode, mixed): each of the log2 N^3 butterfly levels contributes at most
    one rounding of the twiddle constant and one of the product to a term of unit weight, so an output is off by at most
    2 eps log2 N^3 times the modulus it would have if all its terms added coherently; for an impulse that is |want| itself (1
    everywhere), for the others the largest |want| of the case stands for it (attained where the terms do add coherently);
    eps = 2^-24 / 2^-53, the unit roundoff of the storage type.  The mixed case (random x impulse x Nyquist) is here and not
    with the random ones because its transform lives on the single plane k_z = N/2: the rms over the whole cube, which the
    random convention scales by, is sqrt(N) below the values that are there, and those are sums of N equal-weight terms along
    y and z of which the coherent bound is the statement.  For the single mode the peak's scale holds for every output, so
    errors away from the two peaks are left to the rms bound;
  rms, every case: 3 x the rms error of scipy's transform of the same precision at 256^3 (`yardstick`), scaled by
    sqrt(log2 N^3 / 24), times rms(want)."""
import functools

import numpy as np

CASES = ("random", "two_term", "impulse_origin", "impulse_a", "impulse_b", "nyquist", "single_mode", "mixed")
STRUCTURED = ("impulse_origin", "impulse_a", "impulse_b", "nyquist", "single_mode", "mixed")
TOL_RANDOM = {"f32": 3e-6, "f64": 1e-13}
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}


def _q8(v):
    """round to 8 significant bits: integers in [-127, 127] over 128"""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) * 128.), -127, 127) / 128.


def _random_factor(rs, N):
    return rs.randint(-127, 128, size=N).astype(np.float64) / 128.


def _impulse(N, i):
    v = np.zeros(N)
    v[i] = 1.0
    return v


def _nyquist(N):
    return 1.0 - 2.0 * (np.arange(N) % 2)


def single_mode_index(N):
    m = max(1, N // 8 - 1)
    return m, N - m, N // 2 - 1


def case_terms(name, N, seed=0):
    """The terms [(a, b, c), ...] of case `name` on an N^3 grid."""
    rs = np.random.RandomState(1000 * seed + CASES.index(name))
    H = N // 2
    if name == "random":
        return [tuple(_random_factor(rs, N) for _ in range(3))]
    if name == "two_term":
        even = (np.arange(N) % 2 == 0).astype(np.float64)
        t1 = (_random_factor(rs, N) * even, _random_factor(rs, N), _random_factor(rs, N))
        t2 = (_random_factor(rs, N) * (1.0 - even), _random_factor(rs, N), _random_factor(rs, N))
        return [t1, t2]
    if name == "impulse_origin":
        return [(_impulse(N, 0), _impulse(N, 0), _impulse(N, 0))]
    if name == "impulse_a":
        return [(_impulse(N, 1), _impulse(N, N - 1), _impulse(N, H + 1))]
    if name == "impulse_b":
        return [(_impulse(N, N - 1), _impulse(N, H), _impulse(N, 1))]
    if name == "nyquist":
        return [(_nyquist(N), _nyquist(N), _nyquist(N))]
    if name == "single_mode":
        # cos(A + B + C) = cA cB cC - cA sB sC - sA cB sC - sA sB cC with the sines and cosines rounded to 8 bits; A carries
        # a phase of 0.6 rad, so that the two peaks of the transform are neither real nor imaginary
        i = np.arange(N)
        cs = [(_q8(np.cos(2. * np.pi * m * i / N + ph)), _q8(np.sin(2. * np.pi * m * i / N + ph)))
              for m, ph in zip(single_mode_index(N), (0.6, 0., 0.))]
        (ca, sa), (cb, sb), (cc, sc) = cs
        return [(ca, cb, cc), (-ca, sb, sc), (-sa, cb, sc), (-sa, sb, cc)]
    if name == "mixed":
        return [(_random_factor(rs, N), _impulse(N, (3 * N) // 4 + 1), _nyquist(N))]
    raise ValueError(name)


def factor_spectra(terms):
    """[(fft(a), fft(b), fft(c)), ...]: complex128 vectors of the unnormalised forward transform (numpy's sign)."""
    return [tuple(np.fft.fft(v) for v in t) for t in terms]


def field_plane(terms, i):
    """x-plane i of the field, (N, N) float64"""
    return sum(t[0][i] * np.outer(t[1], t[2]) for t in terms)


def spectrum_plane(fterms, i, nz=None):
    """x-plane i of the spectrum from factor_spectra's output, (N, nz) complex128 (nz = N/2+1: the stored half)"""
    return sum(f[0][i] * np.outer(f[1], f[2][:nz]) for f in fterms)


def field(terms):
    """the whole field (small N only)"""
    return np.stack([field_plane(terms, i) for i in range(terms[0][0].size)])


def spectrum(fterms, nz=None):
    """the whole spectrum (small N only)"""
    return np.stack([spectrum_plane(fterms, i, nz) for i in range(fterms[0][0].size)])


def complex_pairs():
    """(real-part case, imaginary-part case) of every complex input: each case appears once in each role"""
    return [(CASES[i], CASES[(i + 3) % len(CASES)]) for i in range(len(CASES))]


# ---- the yardstick of the rms bounds: an independent transform of the same precision ----------------------------------------
@functools.lru_cache(maxsize=None)
def yardstick(precision, n=256, seed=5):
    """(rms, max) error, relative to the rms of the exact spectrum, of scipy's (pocketfft) n^3 transform in `precision`:
    'f32': of an exactly representable float32 random cube, against numpy's fp64 fftn of the same cube;
    'f64': of a separable random cube in double, against the outer product of its long-double 1-D transforms."""
    import scipy.fft
    rs = np.random.RandomState(seed)
    if precision == "f32":
        x = (rs.randint(-2 ** 23, 2 ** 23, size=(n, n, n)).astype(np.float64) / 2. ** 23).astype(np.float32)
        got = scipy.fft.fftn(x)
        assert got.dtype == np.complex64
        err = got.astype(np.complex128)
        del got
        want = np.fft.fftn(x.astype(np.float64))
        err -= want
    else:
        fac = [_random_factor(rs, n) for _ in range(3)]
        x = fac[0][:, None, None] * fac[1][None, :, None] * fac[2][None, None, :]
        err = scipy.fft.fftn(x).astype(np.clongdouble)
        fa, fb, fc = [scipy.fft.fft(v.astype(np.longdouble)) for v in fac]
        assert fa.dtype == np.clongdouble and np.finfo(np.longdouble).eps < 2e-19
        want = fa[:, None, None] * fb[None, :, None] * fc[None, None, :]
        err -= want
    scale = np.sqrt(float(np.mean(np.abs(want) ** 2)))
    return float(np.sqrt(np.mean(np.abs(err) ** 2))) / scale, float(np.max(np.abs(err))) / scale


def rms_bound(precision, N):
    """the yardstick at 256^3 (24 butterfly levels), scaled to log2 N^3 levels (rounding errors add in quadrature), times 3:
    pocketfft's radices and twiddles are not these kernels', and the hardware sine / cosine are not correctly rounded"""
    return 3.0 * yardstick(precision)[0] * np.sqrt(np.log2(float(N) ** 3) / 24.0)


def max_bound(precision, N, name, rms_want, max_want):
    """absolute bound on the largest error of case `name` (module docstring)"""
    levels = np.log2(float(N) ** 3)
    if name in STRUCTURED:
        return 2.0 * EPS[precision] * levels * max_want
    return TOL_RANDOM[precision] * rms_want * np.sqrt(levels)


def check(got, want, precision, name, label=""):
    """numpy form of the comparison the GPU tests make chunk by chunk: asserts both bounds, returns (max err, rms err)."""
    N = want.shape[0]
    err = np.abs(np.asarray(got, dtype=np.complex128) - want)
    rms_want, max_want = np.sqrt(np.mean(np.abs(want) ** 2)), np.max(np.abs(want))
    emax, erms = float(err.max()), float(np.sqrt(np.mean(err ** 2)))
    bmax, brms = max_bound(precision, N, name, rms_want, max_want), rms_bound(precision, N) * rms_want
    assert emax <= bmax, "%s %s max error %.3e > %.3e" % (label, name, emax, bmax)
    assert erms <= brms, "%s %s rms error %.3e > %.3e" % (label, name, erms, brms)
    return emax, erms
