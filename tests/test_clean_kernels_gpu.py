"""GPU: every instance of the NMF and FastICA kernels on the constructed cases of tests/clean_cases.py, through the C entries.

The exact cases carry no tolerance: every sum is exact in any order, so the device must give the bits of the numpy value.
Outputs are pre-filled with NaN, so an element that is not written shows; every call is made twice and must repeat bit for bit.
Three quantities are not exact and follow the rule of tests/test_cleaning_gpu.py (device deviation <= 10 delta_ref, floor 1e-12,
relative to the largest magnitude): the H half of fb_nmf_sweep and its violation (it divides by entries of W^T W; delta_ref = the
float64 reference against its long double evaluation, both on the exact X^T W and W^T W, so a wrong element of either sum moves H
by O(1)), and fb_ica_step with logcosh and exp (delta_ref = the reference's deviation under a fixed permutation of the pixels).

Sizes: tests/clean_cases.py, SWEEP_SIZES -- k_nmf_sweep<T, CPL> and k_nmf_residual<T, CPL> at 1, 2, 4, 8 and 16 channels per lane,
with full and with partly filled last lane groups.  512, 540 and 1000 run in single precision only, on cubes and references built
on the device.  The 32-channel instance of k_nmf_residual (N = 2048) is out of scope: a 2048^3 cube is not a few-second test."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, _lib
from tests import clean_cases as cc
from tests import cleaning_numpy as cn

pytestmark = pytest.mark.gpu
FLOOR = 1e-12
P_i64 = ctypes.POINTER(ctypes.c_int64)


def _box(N, prec):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec)


@functools.lru_cache(maxsize=None)
def _num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _up(eng, x):
    """(npix, N) host matrix -> the device cube in the plan's precision."""
    N = eng.N
    return eng.upload(np.asarray(x).reshape(N, N, N).astype(eng.rdtype), "real")


def _dl(eng, buf, shape, dtype=np.float64):
    h = np.empty(shape, dtype=dtype)
    _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), buf.ptr, h.nbytes, eng.stream)
    eng.sync()
    return h


def _nan(eng, count, dtype=np.float64):
    return eng.upload_raw(np.full(count, np.nan, dtype=dtype))


def _pd(a):
    return a.ctypes.data_as(_lib.P_double)


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d differ, first at %s: device %r, expected %r" % (
            what, len(bad), got.size, i, got[i], want[i]))


def _within(what, got, want, dref):
    scale = float(np.max(np.abs(want)))
    dev = float(np.max(np.abs(np.asarray(got) - want))) / scale if scale else float(np.max(np.abs(got)))
    print("%s: device deviation %.3e, delta_ref %.3e" % (what, dev, dref))
    assert dev <= max(10. * dref, FLOOR), "%s: device deviation %.3e, delta_ref %.3e" % (what, dev, dref)


def _set_row(eng, cube, p, spectrum):
    row = np.ascontiguousarray(spectrum, dtype=eng.rdtype)
    _lib.call("fb_memcpy_h2d", cube.ptr + p * row.nbytes, row.ctypes.data_as(ctypes.c_void_p), row.nbytes, eng.stream)
    eng.sync()                                                       # `row` is this call's


def _params(table, only_f32=()):
    out = []
    for key, sizes in table.items():
        for N in sizes:
            if N in only_f32:
                continue
            out += [pytest.param(key, N, prec, id="cpl%s-%d-%s" % (key, N, prec)) for prec in ("f64", "f32")]
    return out


@functools.lru_cache(maxsize=1)
def _x64(N):
    x = cc.nn_cube(N).astype(np.float64)
    x.setflags(write=False)
    return x


# ---- fb_nmf_sweep ------------------------------------------------------------------------------------------------------------------
def _sweep(eng, cube_ptr, W0, H0):
    """One call from (W0, H0), made twice: (W, H, violations) of the first, after asserting that the second repeats it."""
    k, npix, N = W0.shape[0], W0.shape[1], eng.N
    runs = []
    for _ in range(2):
        W_buf, H_buf, v = eng.upload_raw(W0), eng.upload_raw(H0), np.full(2, np.nan)
        _lib.call("fb_nmf_sweep", eng._plan, cube_ptr, W_buf.ptr, H_buf.ptr, k, _pd(v), eng.stream)
        runs.append((_dl(eng, W_buf, (k, npix)), _dl(eng, H_buf, (k, N)), v))
    for a, b, name in zip(runs[0], runs[1], ("W", "H", "violations")):
        assert a.tobytes() == b.tobytes(), "%s: two calls differ" % name
    return runs[0]


def _check_sweep(what, got, XHt, XtW_of, W0, H0):
    """XtW_of(W) -> the exact X^T W [N][k] of the expected W."""
    W, H, v = got
    want_W, want_viol = cc.expected_w_half(XHt, W0, H0)
    _same("W, " + what, W, want_W)
    assert v[0] == want_viol, "violation of the W half, %s: device %r, expected %r" % (what, v[0], want_viol)
    want_H, want_vh, dref_h, dref_v = cc.h_half(XtW_of(want_W), want_W @ want_W.T, H0)
    _within("H, " + what, H, want_H, dref_h)
    _within("violation of the H half, " + what, v[1:], np.array([want_vh]), dref_v)


@pytest.mark.parametrize("cpl,N,prec", _params(cc.SWEEP_SIZES, cc.F32_ONLY))
def test_nmf_sweep_is_exact(cpl, N, prec):
    assert cc.channels_per_lane(N) == cpl
    eng = _box(N, prec).engine
    x = _x64(N)
    cube = _up(eng, x)
    cases = [("disjoint", k) for k in cc.SWEEP_K] + [("overlap", k) for k in cc.OVERLAP_K if N in cc.OVERLAP_SIZES]
    for design, k in cases:
        W0, H0 = cc.w_start(k, N * N), cc.H_START[design](N, k)
        _check_sweep("design %s, k = %d" % (design, k), _sweep(eng, cube.ptr, W0, H0), x @ H0.T, lambda W: x.T @ W.T, W0, H0)


@pytest.mark.parametrize("N,prec", [(N, prec) for N in cc.HOT_SIZES for prec in ("f64", "f32")])
def test_nmf_sweep_of_one_hot_pixel(N, prec):
    """W = (v H^T) / hess at the hot pixel and 0 elsewhere, X^T W = v W[:, p]^T, wherever the pixel lies in the workgroups' shares."""
    eng = _box(N, prec).engine
    npix, k = N * N, 3
    nb, per = cc.sweep_plan(N, _num_cu())
    positions = cc.sweep_positions(N, nb, per)
    assert len(positions) >= 7 and all(0 <= p < npix for p in positions.values())
    cube = _up(eng, np.zeros((npix, N)))
    v = cc.hot_spectrum(N)
    designs = ["disjoint"] + (["overlap"] if N in cc.OVERLAP_SIZES else [])
    for where, p in positions.items():
        _set_row(eng, cube, p, v)
        for design in designs:
            W0, H0 = cc.w_start(k, npix), cc.H_START[design](N, k)
            XHt = np.zeros((npix, k))
            XHt[p] = H0 @ v
            what = "hot pixel %d (%s; %d workgroups of %d), design %s" % (p, where, nb, per, design)
            _check_sweep(what, _sweep(eng, cube.ptr, W0, H0), XHt, lambda W: cc.one_hot_sums(N, p, W), W0, H0)
        _set_row(eng, cube, p, np.zeros(N))


# ---- fb_nmf_residual ---------------------------------------------------------------------------------------------------------------
def _blank(eng, out):
    blank = np.full(eng.N ** 3, np.nan, dtype=eng.rdtype)
    _lib.call("fb_memcpy_h2d", out.ptr, blank.ctypes.data_as(ctypes.c_void_p), blank.nbytes, eng.stream)
    eng.sync()                                                       # `blank` is this call's


@pytest.mark.parametrize("cpl,N,prec", _params(cc.SWEEP_SIZES, cc.F32_ONLY))
def test_nmf_residual_is_exact(cpl, N, prec):
    assert cc.channels_per_lane(N) == cpl
    eng = _box(N, prec).engine
    npix = N * N
    x = _x64(N)
    cube = _up(eng, x)
    out = eng.empty("real")
    for k in cc.RESIDUAL_K:
        W, H = cc.residual_factors(N, k)
        want, want_ss = cc.expected_residual(x, W, H)
        W_buf, H_buf = eng.upload_raw(W), eng.upload_raw(H)
        for with_out, with_ss in ((True, True), (True, True), (True, False), (False, True)):
            ss = ctypes.c_double(np.nan)
            _blank(eng, out)
            _lib.call("fb_nmf_residual", eng._plan, cube.ptr, W_buf.ptr, H_buf.ptr, k, out.ptr if with_out else None,
                      ctypes.byref(ss) if with_ss else None, eng.stream)
            what = "k = %d, cube_out %s, sumsq_out %s" % (k, "given" if with_out else "NULL", "given" if with_ss else "NULL")
            got = _dl(eng, out, (npix, N), eng.rdtype)
            if with_out:
                _same("residual, " + what, got, want.astype(eng.rdtype))
            else:
                assert np.all(np.isnan(got)), "cube_out = NULL, but a cube was written"
            if with_ss:
                assert ss.value == want_ss, "sum of squares, %s: device %r, expected %r" % (what, ss.value, want_ss)


# ---- 512, 540, 1000: single precision, the cube and the references built on the device -------------------------------------------------
def _device_cube(N):
    """(torch, int8 (npix, N) tensor like clean_cases.nn_cube, the float32 cube)."""
    import torch
    dev = torch.device("cuda", 0)
    npix = N * N
    gen = torch.Generator(device=dev)
    gen.manual_seed(4000 + N)
    x8 = torch.randint(0, cc.XMAX + 1, (npix, N), dtype=torch.int8, device=dev, generator=gen)
    x8 *= torch.from_numpy(np.where(cc.negated(npix), -1, 1).astype(np.int8)).to(dev)[:, None]
    return torch, x8, x8.to(torch.float32)


def _chunks(npix, N):
    step = max(1, (1 << 26) // N)                                   # <= 2^26 doubles (512 MB) per temporary
    return [(a, min(a + step, npix)) for a in range(0, npix, step)]


def _t_same(torch, what, got, want):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(j) for j in bad[0])
        raise AssertionError("%s: %d of %d differ, first at %s: device %r, expected %r" % (
            what, len(bad), got.numel(), i, got[i].item(), want[i].item()))


@pytest.mark.parametrize("N", cc.F32_ONLY)
def test_nmf_sweep_is_exact_on_device_built_cubes(N):
    """cpl = 8 with every lane group full (512), cpl = 16 with 9 (540) and with all 16 lane groups (1000), the last one partial."""
    eng = _box(N, "f32").engine
    torch, x8, cube = _device_cube(N)
    dev, npix = x8.device, N * N
    for k in cc.LARGEST_K.get(N, cc.SWEEP_K):
        W0, H0 = cc.w_start(k, npix), cc.h_disjoint(N, k)
        W0_t, Ht = torch.from_numpy(W0).to(dev), torch.from_numpy(np.ascontiguousarray(H0.T)).to(dev)
        XHt = torch.empty((npix, k), dtype=torch.float64, device=dev)
        for a, b in _chunks(npix, N):
            XHt[a:b] = x8[a:b].double() @ Ht
        want_W, want_viol = cc.cd_pass(XHt, W0_t, (H0 @ H0.T).tolist(), xp=torch)
        XtW = torch.zeros((N, k), dtype=torch.float64, device=dev)
        for a, b in _chunks(npix, N):
            XtW += x8[a:b].double().T @ want_W[:, a:b].T
        WtW = (want_W @ want_W.T).cpu().numpy()
        want_H, want_vh, dref_h, dref_v = cc.h_half(XtW.cpu().numpy(), WtW, H0)
        last = None
        for _ in range(2):
            W_t, H_t, v = W0_t.clone(), torch.from_numpy(H0).to(dev), np.full(2, np.nan)
            torch.cuda.synchronize()
            _lib.call("fb_nmf_sweep", eng._plan, cube.data_ptr(), W_t.data_ptr(), H_t.data_ptr(), k, _pd(v), eng.stream)
            eng.sync()
            state = (W_t, H_t.cpu().numpy(), v)
            if last is not None:
                assert torch.equal(last[0], W_t) and last[1].tobytes() == state[1].tobytes() and last[2].tobytes() == v.tobytes(), \
                    "two calls differ"
            last = state
        what = "N = %d, k = %d" % (N, k)
        _t_same(torch, "W, " + what, last[0], want_W)
        assert last[2][0] == float(want_viol), "violation of the W half, %s: device %r, expected %r" % (
            what, last[2][0], float(want_viol))
        _within("H, " + what, last[1], want_H, dref_h)
        _within("violation of the H half, " + what, last[2][1:], np.array([want_vh]), dref_v)


@pytest.mark.parametrize("N", cc.F32_ONLY)
def test_nmf_residual_is_exact_on_device_built_cubes(N):
    eng = _box(N, "f32").engine
    torch, x8, cube = _device_cube(N)
    dev, npix, k = x8.device, N * N, 5
    W, H = cc.residual_factors(N, k)
    W_t, H_t = torch.from_numpy(W).to(dev), torch.from_numpy(H).to(dev)
    for with_out, with_ss in ((True, True), (True, False), (False, True)):
        out = torch.full((npix, N), float("nan"), dtype=torch.float32, device=dev)
        ss = ctypes.c_double(np.nan)
        torch.cuda.synchronize()
        _lib.call("fb_nmf_residual", eng._plan, cube.data_ptr(), W_t.data_ptr(), H_t.data_ptr(), k,
                  out.data_ptr() if with_out else None, ctypes.byref(ss) if with_ss else None, eng.stream)
        eng.sync()
        want_ss = 0.
        for a, b in _chunks(npix, N):
            want = x8[a:b].double() - W_t[:, a:b].T @ H_t
            want_ss += float((want * want).sum())
            if with_out:
                _t_same(torch, "residual, pixels %d .. %d" % (a, b), out[a:b].double(), want)
        if not with_out:
            assert bool(torch.isnan(out).all()), "cube_out = NULL, but a cube was written"
        if with_ss:
            assert ss.value == want_ss, "sum of squares: device %r, expected %r" % (ss.value, want_ss)
        del out


# ---- fb_ica_step -------------------------------------------------------------------------------------------------------------------
def _ica_step(eng, W, X1_buf, fun, alpha=1.):
    n = len(W)
    runs = []
    for _ in range(2):
        G, gp = np.full((n, n), np.nan), np.full(n, np.nan)
        _lib.call("fb_ica_step", eng._plan, _pd(W), X1_buf.ptr, n, cc.FUN[fun], alpha, _pd(G), _pd(gp), eng.stream)
        runs.append((G, gp))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), "two calls differ"
    return runs[0]


def _plain_params(sizes):
    return [(N, prec) for N in sizes for prec in (("f32",) if N in cc.F32_ONLY else ("f64", "f32"))]


@pytest.mark.parametrize("N,prec", _plain_params(cc.ICA_SIZES))
def test_ica_step_with_the_cube_contrast_is_exact(N, prec):
    eng = _box(N, prec).engine
    npix = N * N
    nb, per = cc.ica_plan(N)
    for n in cc.ICA_N:
        W, X1 = cc.ica_inputs(n, npix)
        want_G, want_gp = cc.expected_ica_cube(W, X1)
        G, gp = _ica_step(eng, W, eng.upload_raw(X1), "cube")
        _same("G, n = %d" % n, G, want_G)
        _same("mean of g', n = %d" % n, gp, want_gp)
        if N in cc.F32_ONLY:
            continue
        X1_buf = eng.upload_raw(np.zeros((n, npix)))                # one hot pixel
        v = cc.ica_hot_vector(W)
        want_G, want_gp = cc.expected_ica_cube_one_hot(W, v, npix)
        for where, p in cc.ica_positions(N, nb, per).items():
            for j in range(n):
                _set_column(eng, X1_buf, npix, j, p, v[j])
            G, gp = _ica_step(eng, W, X1_buf, "cube")
            what = "n = %d, hot pixel %d (%s; %d workgroups of %d)" % (n, p, where, nb, per)
            _same("G, " + what, G, want_G)
            _same("mean of g', " + what, gp, want_gp)
            for j in range(n):
                _set_column(eng, X1_buf, npix, j, p, 0.)


def _set_column(eng, buf, npix, j, p, value):
    one = np.array([value], dtype=np.float64)
    _lib.call("fb_memcpy_h2d", buf.ptr + (j * npix + p) * 8, one.ctypes.data_as(ctypes.c_void_p), 8, eng.stream)
    eng.sync()                                                       # `one` is this call's


@pytest.mark.parametrize("fun,alpha", [("logcosh", 1.), ("logcosh", 1.5), ("exp", 1.)])
@pytest.mark.parametrize("N", cc.REAL_ICA_SIZES)
def test_ica_step_with_logcosh_and_exp(N, fun, alpha):
    eng = _box(N, "f64").engine
    npix = N * N
    pm = np.random.RandomState(99).permutation(npix)
    for n in (2, 16):
        W, X1 = cc.real_ica_inputs(n, npix)

        def ref(x1):
            g, gp = cn.contrast(fun, W @ x1, alpha)
            return g @ x1.T / float(npix), gp
        (want_G, want_gp), (alt_G, alt_gp) = ref(X1), ref(np.ascontiguousarray(X1[:, pm]))
        G, gp = _ica_step(eng, W, eng.upload_raw(X1), fun, alpha)
        what = "N = %d, n = %d, %s, alpha = %g" % (N, n, fun, alpha)
        _within("G, " + what, G, want_G, float(np.max(np.abs(alt_G - want_G)) / np.max(np.abs(want_G))))
        _within("mean of g', " + what, gp, want_gp, float(np.max(np.abs(alt_gp - want_gp)) / np.max(np.abs(want_gp))))


# ---- fb_ica_sources ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec", _plain_params(cc.ICA_SIZES))
def test_ica_sources_are_exact(N, prec):
    eng = _box(N, prec).engine
    npix = N * N
    for n in cc.SOURCES_N:
        W, X1 = cc.ica_inputs(n, npix)
        scale = cc.source_scale(n)
        want_S, want_mom = cc.expected_sources(W, scale, X1)
        X1_buf = eng.upload_raw(X1)
        first = None
        for with_mom in (True, True, False):
            S_buf, mom = _nan(eng, n * npix), np.full(2 * n, np.nan)
            _lib.call("fb_ica_sources", eng._plan, _pd(W), _pd(scale), X1_buf.ptr, n, S_buf.ptr, _pd(mom) if with_mom else None,
                      eng.stream)
            S = _dl(eng, S_buf, (n, npix))
            what = "n = %d, moments_out %s" % (n, "given" if with_mom else "NULL")
            _same("sources, " + what, S, want_S)
            if with_mom:
                _same("moments, " + what, mom, want_mom)
                if first is not None:
                    assert first == (S.tobytes(), mom.tobytes()), "two calls differ"
                first = (S.tobytes(), mom.tobytes())
            else:
                assert np.all(np.isnan(mom))


# ---- fb_real_min -------------------------------------------------------------------------------------------------------------------
def _real_min(eng, cube):
    runs = []
    for _ in range(2):
        mn, bad = ctypes.c_double(np.nan), ctypes.c_int64(-1)
        _lib.call("fb_real_min", eng._plan, cube.ptr, ctypes.byref(mn), ctypes.byref(bad), eng.stream)
        runs.append((mn.value, bad.value))
    assert runs[0] == runs[1] or (np.isnan(runs[0][0]) and np.isnan(runs[1][0])), "two calls differ: %r" % (runs,)
    return runs[0]


def _set_value(eng, cube, i, value):
    one = np.array([value], dtype=eng.rdtype)
    _lib.call("fb_memcpy_h2d", cube.ptr + i * one.nbytes, one.ctypes.data_as(ctypes.c_void_p), one.nbytes, eng.stream)
    eng.sync()                                                       # `one` is this call's


@pytest.mark.parametrize("N,prec", _plain_params(cc.PLAIN_SIZES))
def test_real_min_finds_the_minimum_and_counts_what_is_not_finite(N, prec):
    eng = _box(N, prec).engine
    n = N ** 3
    base = cc.min_base(n, eng.rdtype)
    cube = eng.upload(base.reshape(N, N, N), "real")
    assert _real_min(eng, cube) == (3., 0)
    positions = cc.min_positions(n)
    for where, i in positions.items():
        _set_value(eng, cube, i, -5.)
        assert _real_min(eng, cube) == (-5., 0), "the minimum at %d (%s)" % (i, where)
        for value in (np.nan, np.inf):
            _set_value(eng, cube, i, value)
            got = _real_min(eng, cube)                              # the base holds its least value, 3, every 1000 elements
            assert got == (3., 1), "%r at %d (%s): %r" % (value, i, where, got)
        _set_value(eng, cube, i, -np.inf)
        assert _real_min(eng, cube) == (-np.inf, 1), "-inf at %d (%s)" % (i, where)
        _set_value(eng, cube, i, base[i])
    values = (np.nan, np.inf, -np.inf)                              # all the places at once
    for j, i in enumerate(positions.values()):
        _set_value(eng, cube, i, values[j % 3])
    assert _real_min(eng, cube) == (-np.inf, len(positions))
    cube = eng.upload(np.full((N, N, N), np.nan), "real")
    assert _real_min(eng, cube) == (np.inf, n), "a cube of NaN"


# ---- fb_complex_to_real ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,prec", _plain_params(cc.PLAIN_SIZES))
def test_complex_to_real_takes_the_real_parts(N, prec):
    eng = _box(N, prec).engine
    n = N ** 3
    re = cc.distinct_reals(n, eng.rdtype)
    full = np.empty((n, 2), dtype=eng.rdtype)
    full[:, 0], full[:, 1] = re, np.nan
    full_buf = eng.upload_raw(full)
    bits = np.uint32 if prec == "f32" else np.uint64
    for _ in range(2):
        out = eng.empty("real")
        _blank(eng, out)
        _lib.call("fb_complex_to_real", eng._plan, full_buf.ptr, out.ptr, eng.stream)
        _same("real parts", _dl(eng, out, (n,), eng.rdtype).view(bits), re.view(bits))


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_touch_nothing():
    N = 16
    npix = N * N
    eng = _box(N, "f64").engine
    lib = _lib.load()
    plan, st = eng._plan, eng.stream
    cube = _up(eng, cc.nn_cube(N))
    W_buf, H_buf, X1_buf, S_buf = _nan(eng, 17 * npix), _nan(eng, 17 * N), _nan(eng, 17 * npix), _nan(eng, 17 * npix)
    out = eng.empty("real")
    _blank(eng, out)
    v, ss = np.full(2, np.nan), ctypes.c_double(np.nan)
    Wm, scale, G, gp, mom = np.eye(17), np.ones(17), np.full((17, 17), np.nan), np.full(17, np.nan), np.full(34, np.nan)
    mn, bad = ctypes.c_double(np.nan), ctypes.c_int64(-7)
    calls = []
    for k in (0, 17, -1):
        calls += [("sweep k = %d" % k, lib.fb_nmf_sweep(plan, cube.ptr, W_buf.ptr, H_buf.ptr, k, _pd(v), st)),
                  ("residual k = %d" % k, lib.fb_nmf_residual(plan, cube.ptr, W_buf.ptr, H_buf.ptr, k, out.ptr, ctypes.byref(ss), st)),
                  ("ica_step n = %d" % k, lib.fb_ica_step(plan, _pd(Wm), X1_buf.ptr, k, 2, 1., _pd(G), _pd(gp), st)),
                  ("ica_sources n = %d" % k, lib.fb_ica_sources(plan, _pd(Wm), _pd(scale), X1_buf.ptr, k, S_buf.ptr, _pd(mom), st))]
    for fun in (-1, 3):
        calls.append(("ica_step fun = %d" % fun, lib.fb_ica_step(plan, _pd(Wm), X1_buf.ptr, 3, fun, 1., _pd(G), _pd(gp), st)))
    sweep = [plan, cube.ptr, W_buf.ptr, H_buf.ptr, 3, _pd(v), st]
    residual = [plan, cube.ptr, W_buf.ptr, H_buf.ptr, 3, out.ptr, ctypes.byref(ss), st]
    step = [plan, _pd(Wm), X1_buf.ptr, 3, 2, 1., _pd(G), _pd(gp), st]
    sources = [plan, _pd(Wm), _pd(scale), X1_buf.ptr, 3, S_buf.ptr, _pd(mom), st]
    rmin = [plan, cube.ptr, ctypes.byref(mn), ctypes.byref(bad), st]
    c2r = [plan, S_buf.ptr, out.ptr, st]
    for name, fn, args, nulls in (("sweep", lib.fb_nmf_sweep, sweep, (0, 1, 2, 3, 5)),
                                  ("residual", lib.fb_nmf_residual, residual, (0, 1, 2, 3)),
                                  ("ica_step", lib.fb_ica_step, step, (0, 1, 2, 6, 7)),
                                  ("ica_sources", lib.fb_ica_sources, sources, (0, 1, 2, 3, 5)),
                                  ("real_min", lib.fb_real_min, rmin, (0, 1, 2, 3)),
                                  ("complex_to_real", lib.fb_complex_to_real, c2r, (0, 1, 2))):
        for i in nulls:
            a = list(args)
            a[i] = None
            calls.append(("%s, argument %d null" % (name, i), fn(*a)))
    a = list(residual)
    a[5] = a[6] = None
    calls.append(("residual, both outputs null", lib.fb_nmf_residual(*a)))
    wrong = [(name, code) for name, code in calls if code != -1]     # FB_ERR_INVALID
    assert not wrong, wrong
    eng.sync()
    for name, buf, count in (("W", W_buf, 17 * npix), ("H", H_buf, 17 * N), ("X1", X1_buf, 17 * npix), ("sources", S_buf, 17 * npix),
                             ("cube_out", out, N ** 3)):
        assert np.all(np.isnan(_dl(eng, buf, (count,)))), name + " was written"
    assert np.all(np.isnan(v)) and np.isnan(ss.value) and np.all(np.isnan(G)) and np.all(np.isnan(gp)) and np.all(np.isnan(mom))
    assert np.isnan(mn.value) and bad.value == -7
