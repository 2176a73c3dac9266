"""GPU: the LSSA functions of fastbox_amd.inpaint (fb_lssa) against their numpy statement (tests/lssa_numpy.py).

Tolerances are not fixed in advance.  The statement is evaluated twice, directly in channel order and in reversed order with
the overlap sums from the double-angle identities, on the data as the device stores it (fp32-rounded for an f32 plan); that
deviation, relative to max|A| or max|ps| of the case, is delta_ref.  All device arithmetic is fp64, so a device value may differ
from the statement by 10 delta_ref (floor 1e-12) times that magnitude, whatever the plan's precision.  The averages are held to
the same bound scaled to max|ps_mean| and max|ps_stderr|; n_los is exact.  Every assertion message carries the measured
deviation.

From N = 64 up the per-row statement is evaluated on the constructed rows and a fixed stride of the others (_rows); the averages
are checked over the whole cube through the statement's matrix-product form."""
import functools
import itertools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, inpaint, _lib
from tests import lssa_numpy as ls

pytestmark = pytest.mark.gpu
FLOOR = 1e-12
# 16: one partial tile; 18: a remainder of 2 in the channel sum; 24: a partial channel tile; 64: the first size without edges;
# 128: several tiles per row and several pixel tiles per partial-sum column
SIZES = (16, 18, 24, 64, 128)


@functools.lru_cache(maxsize=None)
def _box(N, prec):
    return CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec)


def _stored(a, prec):
    """what the device holds of a host array"""
    return a.astype(np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _rows(N):
    npix = N * N
    if N < 64:
        return np.arange(npix)
    return np.unique(np.concatenate([np.arange(8), np.arange(8, npix, npix // 248)]))


def _ntaus(N):
    return (1, 5, N, 20 if N == 16 else N + 4)


def _args(c, prec):
    """the case as the device stores it: (d, w, var) for the statement"""
    N = c["N"]
    w = c["w"]
    d = _stored(c["d"], prec)
    d = np.where(np.broadcast_to(w, d.shape) != 0., d, 0.)
    var = c["var"]
    if var is not None and var.ndim == 2:
        var = _stored(var, prec)
    return d, w, var


@functools.lru_cache(maxsize=None)
def _reference(N, prec, per_voxel, noise, taper, ntau, decorrelate=True):
    """(rows, (A_re, A_im, ps) on them, delta_ref of A and of ps with their magnitudes, (mean, stderr, n_los) of the cube)"""
    c = ls.build_case(N, per_voxel, noise, taper)
    d, w, var = _args(c, prec)
    rows, tau = _rows(N), ls.case_tau(N, ntau)
    sub = lambda a: a[rows] if a is not None and a.ndim == 2 else a           # noqa: E731
    a = ls.statement(d[rows], sub(w), sub(var), c["taper"], tau, c["freqs"], decorrelate)
    b = ls.statement(d[rows], sub(w), sub(var), c["taper"], tau, c["freqs"], decorrelate, via="alt")
    dA = max(ls.delta_ref(a[0], b[0])[0], ls.delta_ref(a[1], b[1])[0])
    bigA = max(float(np.max(np.abs(a[0]))), float(np.max(np.abs(a[1]))))
    dP, bigP = ls.delta_ref(a[2], b[2])
    if N < 64:
        avg = ls.averages(a[2], a[3])
    else:
        full = ls.statement(d, w, var, c["taper"], tau, c["freqs"], decorrelate, via="matmul")
        avg = ls.averages(full[2], full[3])
    return rows, a[:3], (dA, bigA), (dP, bigP), avg


def _close(what, got, want, dref, big):
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN in other places" % what
    ok = ~np.isnan(want)
    dev = float(np.max(np.abs(got[ok] - want[ok]))) / big if ok.any() and big > 0. else 0.
    assert dev <= max(10. * dref, FLOOR), "%s: device deviation %.3e (relative to the largest magnitude %.3e), delta_ref %.3e" % (
        what, dev, big, dref)


def _noise_arg(c, form):
    """the variances in the form the call takes them: (N,), a diagonal matrix, or a cube"""
    N, var = c["N"], c["var"]
    if var is None:
        return None
    if var.ndim == 1:
        return np.diag(var) if form else var
    return var.reshape(N, N, N) if form else var


def _run_case(N, prec, per_voxel, noise, taper, ntau, form=False):
    c = ls.build_case(N, per_voxel, noise, taper)
    rows, (a_re, a_im, ps), (dA, bigA), (dP, bigP), (mean, err, n_los) = _reference(N, prec, per_voxel, noise, taper, ntau)
    box = _box(N, prec)
    sp = inpaint.lssa_delay_spectrum(c["d_nan"], c["w"], freqs=c["freqs"], N=_noise_arg(c, form), tau=ls.case_tau(N, ntau),
                                     taper=c["taper"], keep=True, box=box)
    tag = "N = %d, %s, %s flags, noise %s, taper %s, Ntau = %d" % (N, prec, "per-voxel" if per_voxel else "per-channel", noise,
                                                                 taper, ntau)
    g_re, g_im = sp.modes.host()
    g_ps = sp.ps_host()
    assert g_re.shape == g_im.shape == g_ps.shape == (N * N, ntau)
    _close(tag + ": A_re", g_re[rows], a_re, dA, bigA)
    _close(tag + ": A_im", g_im[rows], a_im, dA, bigA)
    _close(tag + ": ps", g_ps[rows], ps, dP, bigP)
    assert sp.n_los == n_los == sp.modes.n_los, "%s: n_los %d, statement %d" % (tag, sp.n_los, n_los)
    assert np.all(np.isfinite(sp.ps_mean)) and np.all(np.isfinite(sp.ps_stderr)), tag
    _close(tag + ": ps_mean", sp.ps_mean, mean, dP, float(np.max(np.abs(mean))))
    _close(tag + ": ps_stderr", sp.ps_stderr, err, dP, float(np.max(np.abs(err))))
    if per_voxel:
        # row 3 is fully flagged: A = 0, ps NaN, not counted
        assert np.array_equal(g_re[3], np.zeros(ntau)) and np.array_equal(g_im[3], np.zeros(ntau)) and np.all(np.isnan(g_ps[3])), tag
        assert n_los == N * N - 1 and np.isnan(g_ps).sum() == ntau, tag
    else:
        assert n_los == N * N and not np.isnan(g_ps).any(), tag
    return sp


_CONFIGS = list(itertools.product((False, True), (None, "chan", "cube"), (False, True)))


@pytest.mark.parametrize("N,prec", list(itertools.product(SIZES, ("f32", "f64"))))
def test_delay_spectrum_matches_the_statement(N, prec):
    """per-channel and per-voxel flags x no variances, per channel, per voxel x taper or none; Ntau cycles through 1, 5, N and one
    value above N, and the two forms of each kind of variance alternate"""
    for i, (per_voxel, noise, taper) in enumerate(_CONFIGS):
        _run_case(N, prec, per_voxel, noise, taper, _ntaus(N)[(i + N // 2) % 4], form=bool(i & 1))
    _run_case(N, prec, False, "cube", True, N)              # (the cycle leaves this instance without Ntau = N)


@pytest.mark.parametrize("N,per_voxel", list(itertools.product(SIZES, (False, True))))
def test_every_number_of_modes(N, per_voxel):
    for ntau in _ntaus(N):
        _run_case(N, "f64", per_voxel, "chan", True, ntau)


@pytest.mark.parametrize("N", (16, 64))
def test_without_the_decorrelation(N):
    c = ls.build_case(N, True, "chan", True)
    ntau = N
    rows, (a_re, a_im, ps), (dA, bigA), (dP, bigP), (mean, err, n_los) = _reference(N, "f64", True, "chan", True, ntau, False)
    sp = inpaint.lssa_delay_spectrum(c["d_nan"], c["w"], freqs=c["freqs"], N=c["var"], tau=ls.case_tau(N, ntau), taper=c["taper"],
                                     decorrelate_amps=False, keep=True, box=_box(N, "f64"))
    g_re, g_im = sp.modes.host()
    _close("ps without the decorrelation", sp.ps_host()[rows], ps, dP, bigP)
    on = ~np.isnan(sp.ps_host()[:, 0])
    assert np.array_equal(sp.ps_host()[on], g_re[on] * g_re[on] + g_im[on] * g_im[on])
    _close("ps_mean", sp.ps_mean, mean, dP, float(np.max(np.abs(mean))))


@pytest.mark.parametrize("N,prec", [(16, "f64"), (24, "f32"), (64, "f64")])
def test_per_channel_flags_as_a_cube_take_the_other_instance(N, prec):
    c = ls.build_case(N, False, "chan", True)
    ntau = N
    rows, (a_re, a_im, ps), (dA, bigA), (dP, bigP), (mean, err, n_los) = _reference(N, prec, False, "chan", True, ntau)
    box = _box(N, prec)
    kw = dict(freqs=c["freqs"], N=c["var"], tau=ls.case_tau(N, ntau), taper=c["taper"], keep=True, box=box)
    a = inpaint.lssa_delay_spectrum(c["d_nan"], c["w"], **kw)
    b = inpaint.lssa_delay_spectrum(c["d_nan"], np.broadcast_to(c["w"], (N * N, N)), **kw)
    for what, sp in (("per channel", a), ("as a cube", b)):
        g_re, g_im = sp.modes.host()
        _close(what + ": A_re", g_re[rows], a_re, dA, bigA)
        _close(what + ": A_im", g_im[rows], a_im, dA, bigA)
        _close(what + ": ps", sp.ps_host()[rows], ps, dP, bigP)
        _close(what + ": ps_mean", sp.ps_mean, mean, dP, float(np.max(np.abs(mean))))
    _close("cube against per channel: ps", b.ps_host(), a.ps_host(), dP, bigP)
    assert a.n_los == b.n_los == N * N


@pytest.mark.parametrize("N,per_voxel", [(18, True), (18, False), (64, True)])
def test_outputs_are_optional_and_calls_repeatable(N, per_voxel):
    c = ls.build_case(N, per_voxel, "cube", True)
    box = _box(N, "f32")
    ntau = N
    inp = inpaint._LSSAInputs(c["d_nan"], c["w"], c["freqs"], c["var"], ls.case_tau(N, ntau), c["taper"], box)
    eng = inp.engine

    def call(use):
        bufs = [inp.rows() if u else None for u in use]
        mean, err, n_los = inp.run(True, *bufs)
        return [inpaint._rows_host(eng, b, ntau) if b is not None else None for b in bufs] + [mean, err, n_los]

    full = call((True, True, True))
    again = call((True, True, True))
    for x, y in zip(full, again):
        assert np.array_equal(x, y, equal_nan=True), "two identical calls differ"
    for drop in range(3):
        use = [True, True, True]
        use[drop] = False
        part = call(use)
        for k, (x, y) in enumerate(zip(full, part)):
            if y is not None:
                assert np.array_equal(x, y, equal_nan=True), "output %d changes when output %d is not stored" % (k, drop)
    none = call((False, False, False))
    assert np.array_equal(none[3], full[3]) and np.array_equal(none[4], full[4]) and none[5] == full[5]


@pytest.mark.parametrize("N,prec,per_voxel", [(16, "f64", True), (24, "f32", False), (64, "f32", True)])
def test_fit_then_pspec_equals_the_fused_call(N, prec, per_voxel):
    c = ls.build_case(N, per_voxel, "chan", True)
    box = _box(N, prec)
    ntau = N
    kw = dict(freqs=c["freqs"], N=c["var"], tau=ls.case_tau(N, ntau), taper=c["taper"], box=box)
    fused = inpaint.lssa_delay_spectrum(c["d_nan"], c["w"], keep=True, **kw)
    modes = inpaint.lssa_fit_modes(c["d_nan"], c["w"], **kw)
    sp = inpaint.lssa_pspec(modes)
    assert np.array_equal(modes.A_re_host(), fused.modes.A_re_host()) and np.array_equal(modes.A_im_host(), fused.modes.A_im_host())
    assert np.array_equal(sp.ps_host(), fused.ps_host(), equal_nan=True)
    assert np.array_equal(sp.ps_mean, fused.ps_mean) and np.array_equal(sp.ps_stderr, fused.ps_stderr)
    assert sp.n_los == fused.n_los == modes.n_los
    # the amplitude / phase form is the same optimum
    ap = inpaint.lssa_fit_modes(c["d_nan"], c["w"], fit_amp_phase=True, **kw)
    amp, phase = ap.host()
    assert np.all((phase >= 0.) & (phase <= 2. * np.pi))
    A = modes.A_re_host() + 1j * modes.A_im_host()
    assert np.max(np.abs(amp * np.exp(1j * phase) - A)) <= 1e-14 * np.max(np.abs(A))
    # the power under the same flags handed over again
    sp2 = inpaint.lssa_pspec(modes, w=c["w"], box=box)
    assert np.array_equal(sp2.ps_host(), sp.ps_host(), equal_nan=True)


def test_a_sinusoid_on_the_delay_grid():
    """an unflagged row holding amp cos(phi_k + phase) returns |A| = amp / 2 at +-tau_k and about 0 elsewhere; with 10 % of the
    channels flagged the leak into the other modes is there and matches the statement"""
    N, k, amp = 64, 5, 1.7
    freqs, tau = ls.case_freqs(N), ls.case_tau(N, N)
    row = amp * np.cos(ls.phase(tau, freqs)[k] + 0.4)
    d = np.tile(row, (N * N, 1))
    box = _box(N, "f64")
    sp = inpaint.lssa_delay_spectrum(d, np.ones(N), freqs=freqs, tau=tau, keep=True, box=box)
    A = np.hypot(*sp.modes.host())[7]
    want = np.zeros(N)
    want[[k, N - k]] = amp / 2.
    # the modes are orthogonal as far as the phases are exact: they are rounded at 2^-53 max|phi|, in each of N terms
    tol = N * 2. ** -52 * float(np.max(np.abs(ls.phase(tau, freqs))))
    assert np.max(np.abs(A - want)) <= tol * amp, "unflagged: |A| deviates from amp / 2 at +-tau_k by %.3e" % np.max(np.abs(A - want))
    w = np.ones(N)
    w[np.random.RandomState(5).choice(N, size=6, replace=False)] = 0.
    sp = inpaint.lssa_delay_spectrum(d, w, freqs=freqs, tau=tau, keep=True, box=box)
    g_re, g_im = sp.modes.host()
    a = ls.statement(d[:8], w, None, None, tau, freqs)
    b = ls.statement(d[:8], w, None, None, tau, freqs, via="alt")
    others = np.delete(np.arange(N), [k, N - k])
    leak = float(np.max(np.hypot(g_re[7], g_im[7])[others]))
    assert leak > 1e-3 * amp, "flagged: the leak into the other modes is %.3e" % leak
    dA = max(ls.delta_ref(a[0], b[0])[0], ls.delta_ref(a[1], b[1])[0])
    _close("flagged sinusoid: A_re", g_re[:8], a[0], dA, float(np.max(np.abs(a[0]))))
    _close("flagged sinusoid: A_im", g_im[:8], a[1], dA, float(np.max(np.abs(a[1]))))
    _close("flagged sinusoid: ps", sp.ps_host()[:8], a[2], *ls.delta_ref(a[2], b[2]))


def test_device_cubes_and_default_arguments():
    """REAL DeviceArrays for d and w, freqs and tau by default: box.freq_array() and lssa_tau of it"""
    N = 16
    c = ls.build_case(N, True)
    box = _box(N, "f64")
    eng = box.engine
    d_dev = eng.upload(c["d_nan"].reshape(N, N, N), "real")
    w_dev = eng.upload(c["w"].reshape(N, N, N), "real")
    sp = inpaint.lssa_delay_spectrum(d_dev, w_dev, keep=True, box=box)
    freqs = np.asarray(box.freq_array(), dtype=np.float64)
    assert np.array_equal(sp.tau, inpaint.lssa_tau(freqs)) and np.array_equal(sp.modes.freqs, freqs)
    d = np.where(c["w"] != 0., c["d"], 0.)
    a = ls.statement(d, c["w"], None, None, sp.tau, freqs)
    b = ls.statement(d, c["w"], None, None, sp.tau, freqs, via="alt")
    _close("default arguments: ps", sp.ps_host(), a[2], *ls.delta_ref(a[2], b[2]))
    mean, err, n = ls.averages(a[2], a[3])
    assert sp.n_los == n
    _close("default arguments: ps_mean", sp.ps_mean, mean, ls.delta_ref(a[2], b[2])[0], float(np.max(np.abs(mean))))


def test_invalid_arguments_of_the_entry_point():
    """wrong kinds, a mode count outside 1 .. 1024 and NULL tables give FB_ERR_INVALID (-1)"""
    N = 16
    c = ls.build_case(N, True)
    inp = inpaint._LSSAInputs(c["d_nan"], c["w"], c["freqs"], None, ls.case_tau(N, 5), None, _box(N, "f64"))
    eng = inp.engine
    good = [eng._plan, inp.d.ptr, inp.w.ptr, 1, None, 0, None, inp.cos.ptr, inp.sin.ptr, None, 5, 1, 0, None, None, None, None, None,
            None, eng.stream]
    _lib.call("fb_lssa", *good)
    for pos, value in ((3, 7), (5, -1), (10, 0), (10, 1025), (7, None), (8, None), (1, None), (2, None)):
        bad = list(good)
        bad[pos] = value
        with pytest.raises(_lib.FastBoxError) as e:
            _lib.call("fb_lssa", *bad)
        assert e.value.code == -1, (pos, value, e.value.code)
    # per-channel flags with the decorrelation need the overlap sums of the host
    wc = eng.upload_raw(np.ones(N))
    bad = list(good)
    bad[2], bad[3] = wc.ptr, 0
    with pytest.raises(_lib.FastBoxError) as e:
        _lib.call("fb_lssa", *bad)
    assert e.value.code == -1
