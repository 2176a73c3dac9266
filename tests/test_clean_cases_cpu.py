"""CPU: the constructed NMF / FastICA cases (tests/clean_cases.py) against independent statements (tests/cleaning_numpy.py and a
fractions.Fraction evaluation), the exact range of every intermediate at every size the GPU tests use, and the two pixel
partitions (fb_nmf_sweep_plan, fb_ica_step_plan)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import clean_cases as cc
from tests import cleaning_numpy as cn
from tests import pca_cases as pc

DESIGNS = [("disjoint", k) for k in cc.SWEEP_K] + [("overlap", k) for k in cc.OVERLAP_K]


def _sweep_case(N, design, k):
    x = cc.nn_cube(N).astype(np.float64)
    H0, W0 = cc.H_START[design](N, k), cc.w_start(k, N * N)
    return x, H0, W0


def _frac_cd_row(v, b, A):
    """The definition on one row, in rationals.  Returns the violation."""
    k = len(v)
    viol = Fraction(0)
    for t in range(k):
        grad = -b[t] + sum(A[t][r] * v[r] for r in range(k))
        viol += abs(min(Fraction(0), grad) if v[t] == 0 else grad)
        if A[t][t] != 0:
            v[t] = max(v[t] - grad / A[t][t], Fraction(0))
    return viol


def _frac(a):
    return [[Fraction(float(v)) for v in row] for row in np.atleast_2d(a)]


@pytest.mark.parametrize("design,k", DESIGNS)
@pytest.mark.parametrize("N", [16, 18])
def test_sweep_expectations_agree_with_independent_statements(N, design, k):
    x, H0, W0 = _sweep_case(N, design, k)
    npix = N * N
    A = H0 @ H0.T
    if design == "disjoint":
        assert np.array_equal(A, np.diag(np.diag(A))) and set(np.unique(H0)) <= {0., 1., 2., 4.}
        d = np.diag(A)
        assert np.all((d == 0.) | (d == 2. ** np.round(np.log2(np.maximum(d, 1.)))))
        assert k == 1 or d[1] == 0.                                                 # hess == 0
        assert np.any(H0[:, N - 1]) and np.all(np.count_nonzero(H0, axis=0) <= 1)      # the last channel; disjoint supports
    else:
        assert np.all(np.diag(A) == 2.) and np.all(np.diag(A, 1) == 1.) and set(np.unique(H0)) == {0., 1.}
        assert H0[0, 0] == 1. and H0[k - 1, N - 1] == 1.
    W, viol = cc.expected_w_half(x @ H0.T, W0, H0)
    # the numpy statement of the filter's tests
    Wn = np.array(W0.T, order="C")
    vn = cn._cd_half(x, Wn, np.ascontiguousarray(H0.T))
    assert np.array_equal(W, Wn.T) and viol == vn
    # the branches smooth positive data does not reach
    grad0 = -(x @ H0.T)[:, 0] + A[0, 0] * W0[0]
    assert np.any((W0[0] == 0.) & (grad0 > 0.)), "v[t] == 0 with a positive gradient"
    assert np.any((W0[0] > 0.) & (W0[0] - grad0 / A[0, 0] < 0.) & (W[0] == 0.)), "a step clipped to 0"
    assert np.any(W0 == 0.) and np.any(W == 0.) and np.any(W > 0.)
    if design == "disjoint" and k > 1:
        assert np.array_equal(W[1], W0[1]), "hess == 0 keeps the coefficient"
    # rationals
    Af, viol_f = _frac(A), Fraction(0)
    xh = _frac(x @ H0.T)
    for p in range(0, npix, 1 if N == 16 else 5):
        v = [Fraction(float(W0[t, p])) for t in range(k)]
        viol_f += _frac_cd_row(v, xh[p], Af)
        assert [Fraction(float(W[t, p])) for t in range(k)] == v, p
    if N == 16:
        assert Fraction(float(viol)) == viol_f
    # the H half: the exact sums, then one pass per channel
    XtW, WtW = x.T @ W.T, W @ W.T
    H, vh, dref_h, dref_v = cc.h_half(XtW, WtW, H0)
    assert dref_h < 1e-14 and dref_v < 1e-14, (dref_h, dref_v)
    Ht = np.array(H0.T, order="C")
    vhn = cn._cd_half(np.ascontiguousarray(x.T), Ht, np.ascontiguousarray(W.T))
    assert np.max(np.abs(H - Ht.T)) <= 1e-13 * np.max(np.abs(H)) and abs(vh - vhn) <= 1e-13 * vh
    if N == 16:
        Wf = _frac(W)
        xf = _frac(x)
        WtWf = [[sum(Wf[t][p] * Wf[r][p] for p in range(npix)) for r in range(k)] for t in range(k)]
        assert [[Fraction(float(v)) for v in row] for row in WtW] == WtWf, "W^T W must be exact"
        viol_f = Fraction(0)
        for c in range(N):
            b = [sum(xf[p][c] * Wf[t][p] for p in range(npix)) for t in range(k)]
            assert [Fraction(float(v)) for v in XtW[c]] == b, "X^T W must be exact"
            v = [Fraction(float(H0[t, c])) for t in range(k)]
            viol_f += _frac_cd_row(v, b, WtWf)
            assert max(abs(float(v[t]) - H[t, c]) for t in range(k)) <= max(10. * dref_h, 1e-12) * np.max(np.abs(H))
        assert abs(float(viol_f) - vh) <= max(10. * dref_v, 1e-12) * vh


@pytest.mark.parametrize("N", [16, 18])
def test_one_hot_sweep_expectations(N):
    npix, k = N * N, 3
    H0, W0, v = cc.h_disjoint(N, k), cc.w_start(k, N * N), cc.hot_spectrum(N)
    assert np.all(v >= 1.) and np.array_equal(v, np.abs(pc.hot_spectrum(N)))
    for p in cc.sweep_positions(N, *cc.sweep_plan(N, 256)).values():
        x = np.zeros((npix, N))
        x[p] = v
        W, viol = cc.expected_w_half(x @ H0.T, W0, H0)
        assert np.array_equal(cc.one_hot_sums(N, p, W), x.T @ W.T)
        others = np.arange(npix) != p
        assert np.all(W[0, others] == 0.) and W[0, p] == (v @ H0[0]) / (H0[0] @ H0[0]) and np.array_equal(W[1], W0[1])


@pytest.mark.parametrize("k", cc.RESIDUAL_K)
def test_residual_expectation(k):
    N = 16
    x = cc.nn_cube(N).astype(np.float64)
    W, H = cc.residual_factors(N, k)
    r, ss = cc.expected_residual(x, W, H)
    tot = 0
    for p in range(N * N):
        for c in range(N):
            want = int(x[p, c]) - sum(int(W[t, p]) * int(H[t, c]) for t in range(k))
            assert r[p, c] == want
            tot += want * want
    assert ss == tot and np.array_equal(r.astype(np.float32).astype(np.float64), r)


@pytest.mark.parametrize("n", sorted(set(cc.ICA_N) | set(cc.SOURCES_N)))
def test_ica_expectations_agree_with_independent_statements(n):
    N = 16
    npix = N * N
    W, X1 = cc.ica_inputs(n, npix)
    assert np.all(np.any(W != 0., axis=1)) and np.abs(W).max() <= 2. and np.abs(X1).max() <= 4.
    G, gp = cc.expected_ica_cube(W, X1)
    g, gpm = cn.contrast("cube", W @ X1)
    assert np.max(np.abs(G - g @ X1.T / float(npix))) <= 4 * np.finfo(float).eps * np.max(np.abs(G))
    assert np.max(np.abs(gp - gpm)) <= 4 * np.finfo(float).eps * np.max(np.abs(gp))
    Wi, Xi = W.astype(np.int64), X1.astype(np.int64)
    for i in range(n):
        y = [sum(int(Wi[i, j]) * int(Xi[j, p]) for j in range(n)) for p in range(npix)]
        for j in range(n):
            assert G[i, j] == float(sum(y[p] ** 3 * int(Xi[j, p]) for p in range(npix))) * (1.0 / npix)
        assert gp[i] == float(sum(3 * y[p] ** 2 for p in range(npix))) * (1.0 / npix)
    v = cc.ica_hot_vector(W)
    assert np.all(v != 0.) and np.abs(v).max() <= 4.
    for p in cc.ica_positions(N, *cc.ica_plan(N)).values():
        hot = np.zeros((n, npix))
        hot[:, p] = v
        Gh, gph = cc.expected_ica_cube(W, hot)
        Go, gpo = cc.expected_ica_cube_one_hot(W, v, npix)
        assert np.array_equal(Gh, Go) and np.array_equal(gph, gpo) and np.all(gpo > 0.)
    scale = cc.source_scale(n)
    assert np.all(np.abs(scale) == 2. ** np.round(np.log2(np.abs(scale)))) and (n < 4 or np.any(scale < 0.))
    S, mom = cc.expected_sources(W, scale, X1)
    for i in range(n):
        row = [Fraction(float(scale[i])) * sum(int(Wi[i, j]) * int(Xi[j, p]) for j in range(n)) for p in range(npix)]
        assert [Fraction(float(s)) for s in S[i]] == row
        assert mom[i] == float(sum(row)) * (1.0 / npix) and mom[n + i] == float(sum(r * r for r in row)) * (1.0 / npix)


def test_min_and_real_part_cases():
    for N in cc.PLAIN_SIZES:
        n = N ** 3
        pos = cc.min_positions(n)
        assert len(set(pos.values())) == len(pos) >= 6 and all(0 <= p < n for p in pos.values())
        assert any("tail" in name for name in pos) == (n > 1024 * 256)
    for dtype in (np.float32, np.float64):
        base = cc.min_base(5000, dtype)
        assert base.min() == 3. and base.max() <= 1002. and np.all(np.isfinite(base))
        r = cc.distinct_reals(270 ** 3, dtype)
        assert r.dtype == dtype and np.all(np.isfinite(r)) and np.all(np.diff(r) > 0.)


def _dyadic(a, frac_bits):
    s = np.asarray(a, dtype=np.float64) * 2. ** frac_bits
    return bool(np.all(s == np.rint(s)))


@pytest.mark.parametrize("N", cc.ALL_SIZES)
def test_every_intermediate_stays_in_the_exact_range(N):
    """Bounds from the constructions alone (no big products): a sum whose terms are multiples of 2^-f and whose absolute values add
    up to less than 2^(53 - f) is exact in fp64 in any order; a stored value with fewer than 24 significant bits is exact in fp32."""
    npix = N * N
    X = float(cc.XMAX)
    assert cc.XMAX < 2 ** 24 and np.abs(cc.hot_spectrum(N)).max() <= X
    assert _dyadic(cc.w_start(3, 256), 2) and cc.w_start(3, 256).max() <= 4.
    ks = cc.LARGEST_K.get(N, cc.SWEEP_K) if any(N in v for v in cc.SWEEP_SIZES.values()) else ()
    for k in ks:
        H0 = cc.h_disjoint(N, k)
        A = H0 @ H0.T
        assert np.array_equal(A, np.diag(np.diag(A)))
        e = int(np.log2(max(np.diag(A).max(), 1.)))
        assert np.diag(A).max() == 2. ** e
        # b = X H^T: integers; grad = -b + hess w0: quarters; the new w = b / hess: multiples of 2^-e, at most XMAX because
        # sum(H) <= sum(H^2); a kept row (hess == 0) holds W0: quarters up to 4
        bmax = X * np.abs(H0).sum(axis=1).max()
        assert np.all(np.abs(H0).sum(axis=1) <= np.diag(A))
        gmax = bmax + 4. * np.diag(A).max()
        assert npix * k * gmax * 4 < 2 ** 53, "the violation"
        f = max(e, 2)
        assert X * 2 ** f < 2 ** 53, "W"
        assert npix * X * X * 2 ** f < 2 ** 53, "X^T W"
        assert npix * X * X * 2 ** (2 * f) < 2 ** 53, "W^T W"
    if N in cc.OVERLAP_SIZES:
        for k in cc.OVERLAP_K:
            # every step: w <- max(b / 2 - neighbours / 2, 0) <= XMAX, one more fraction bit; grad: |b| + 2 w + two neighbours
            f = 2 + k
            assert npix * k * (2 * X + 4 * X) * 2 ** f < 2 ** 53, "the violation"
            assert npix * X * X * 2 ** (2 * f) < 2 ** 53, "X^T W and W^T W"
    # the residual: |x - sum w h| <= XMAX + 4 k, an integer
    rmax = X + 4 * max(cc.RESIDUAL_K)
    assert rmax < 2 ** 24 and npix * N * rmax * rmax < 2 ** 53
    # FastICA: |y| <= 2 * 4 * n; g x = y^3 x; g' = 3 y^2; sources: scale <= 2 with two fraction bits
    ymax = 2. * 4. * cc.KMAX
    assert npix * ymax ** 3 * 4. < 2 ** 53 and npix * 3. * ymax ** 2 < 2 ** 53
    sc = np.abs(cc.source_scale(cc.KMAX))
    assert sc.max() <= 2. and _dyadic(sc, 2)
    assert npix * (2. * ymax) ** 2 * 2 ** 4 < 2 ** 53


# ---- the pixel partitions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cu", pc.NUM_CU)
def test_sweep_partition_covers_every_pixel_once(num_cu):
    for N in pc.supported_sizes():
        npix = N * N
        nb, per = cc.sweep_plan(N, num_cu)
        assert nb == min(npix // 4, 2 * num_cu) and per == (-(-npix // nb) + 3) // 4 * 4, (N, nb, per)
        assert per % 4 == 0 and per >= 4, (N, nb, per)
        shares = [(min(q * per, npix), min((q + 1) * per, npix)) for q in range(nb)]
        assert shares[0][0] == 0 and shares[-1][1] == npix, (N, nb, per)             # with abutting shares: every pixel once
        assert all(shares[q][1] == shares[q + 1][0] for q in range(nb - 1))
        pos = cc.sweep_positions(N, nb, per)
        assert len(set(pos.values())) == len(pos) and all(0 <= p < npix for p in pos.values()), (N, pos)
        names = " / ".join(pos)
        for want in ("first", "last", "mod4=0", "mod4=1", "mod4=2", "mod4=3", "start of the last non-empty workgroup"):
            assert want in names, (N, want)
        if nb > 1:
            assert "end of workgroup 0" in names and "start of workgroup 1" in names


def test_ica_partition_covers_every_pixel_once():
    for N in pc.supported_sizes():
        npix = N * N
        nb, per = cc.ica_plan(N)
        assert nb == min(-(-npix // 64), 1024) and per == -(-npix // nb), (N, nb, per)
        shares = [(min(q * per, npix), min((q + 1) * per, npix)) for q in range(nb)]
        assert shares[0][0] == 0 and shares[-1][1] == npix and all(shares[q][1] == shares[q + 1][0] for q in range(nb - 1))
        pos = cc.ica_positions(N, nb, per)
        assert len(set(pos.values())) == len(pos) and all(0 <= p < npix for p in pos.values()), (N, pos)
        names = " / ".join(pos)
        for want in ("first", "last", "end of workgroup 0", "start of workgroup 1", "p0 + 15", "p0 + 16"):
            assert want in names, (N, want)


def test_the_edges_the_issue_names():
    assert cc.sweep_plan(72, 256) == (512, 12)                                      # workgroups 432 .. 511 are empty
    assert -(-72 * 72 // 12) == 432
    assert cc.ica_plan(18) == (6, 54)                                               # a ragged last step: 54 = 3 * 16 + 6
    nb, per = cc.ica_plan(270)
    assert (nb, per) == (1024, 72) and nb - -(-270 * 270 // per) == 11              # eleven empty trailing workgroups
    assert cc.ica_plan(512)[1] == 256 and cc.ica_plan(270)[1] > 64                  # more than four steps per thread
    assert [cc.channels_per_lane(N) for N in (64, 72, 128, 144, 256, 270, 512, 540, 1000)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    for cpl, sizes in cc.SWEEP_SIZES.items():
        assert all(cc.channels_per_lane(N) == cpl for N in sizes)


def test_plans_reject_bad_arguments():
    from fastbox_amd import _lib
    lib = _lib.load()
    s, r = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.fb_nmf_sweep_plan(16, 256, ctypes.byref(s), ctypes.byref(r)) == 0 and (s.value, r.value) == (64, 4)
    assert lib.fb_nmf_sweep_plan(1, 256, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_nmf_sweep_plan(1026, 256, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_nmf_sweep_plan(16, 0, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_nmf_sweep_plan(16, 256, None, ctypes.byref(r)) != 0
    assert lib.fb_nmf_sweep_plan(16, 256, ctypes.byref(s), None) != 0
    assert lib.fb_ica_step_plan(16, ctypes.byref(s), ctypes.byref(r)) == 0 and (s.value, r.value) == (4, 64)
    assert lib.fb_ica_step_plan(1, ctypes.byref(s), ctypes.byref(r)) != 0
    assert lib.fb_ica_step_plan(16, None, ctypes.byref(r)) != 0
    assert lib.fb_ica_step_plan(16, ctypes.byref(s), None) != 0
