"""GPU: the cosmic-web classification (fb_web.hip; fastbox_amd/web.py; CosmoBox.tidal_tensor, .cosmic_web) on the constructed
cases of tests/web_cases.py, in both precisions, stage by stage against the numpy statement of tests/web_numpy.py -- which
tests/test_web_cases_cpu.py validates on its own -- each stage fed the statement's exact inputs so that errors do not compound:
the tensors from uploaded spectra, the eigenvalues and classes from uploaded component cubes.  Nothing is larger than 32^3;
most cases run at 16^3 and 18^3, the eigen kernel also at 30^3.

Measured eigenvalue error: see the docstring of test_eigenvalues_are_backward_stable."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, DeviceArray, _lib, default_cosmo, hostgeom, web
from fastbox_amd import box as fb_box
from fastbox_amd.device import HALF, REAL
from tests import web_cases as wc
from tests import web_numpy as wn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
TENSOR_TOL = {"f64": 1e-11, "f32": 1e-5}       # of max|T|: the project's parity tolerances for transformed fields (README)
GEOMS = wc.geometries()
GEOM_IDS = ["N%d-%s" % (N, "x".join("%g" % a for a in L)) for N, L in GEOMS]
EIGEN_GEOMS = GEOMS + [(30, (60., 60., 60.))]   # 30^3: tails in every wave
EIGEN_IDS = GEOM_IDS + ["N30-60x60x60"]
SEED = 3


@functools.lru_cache(maxsize=None)
def _box(prec, N, L):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng="device", seed=SEED)


def _upload_half(eng, spec):
    """A half spectrum (N, N, N/2 + 1) as the device stores it: (N, rows, pitch), padding zero."""
    N = eng.N
    raw = np.zeros((N, eng.rows, eng.pitch), dtype=eng.cdtype)
    raw[:, :N, :N // 2 + 1] = spec
    d = eng.empty(HALF)
    _lib.call("fb_memcpy_h2d", d.ptr, raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes, eng.stream)
    eng.sync()
    return d


def _host(tensor):
    return np.array([np.asarray(c) for c in tensor.components])


def _densities(N, L):
    out = {name: wc.plane_wave(N, L, mode)[0] for name, mode in wc.WAVES.items()}
    out["random"] = wc.random_field(N)
    return out


@functools.lru_cache(maxsize=None)
def _random_tensor(N, L, prec):
    """(the statement's tidal tensor of the random field at R = 3 rounded to the plan's precision, the field)"""
    delta = wc.random_field(N)
    return wn.stored(wn.tidal_tensor(delta, L, 3., DT[prec]), DT[prec]), delta


# ---- tensors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_tidal_tensor_is_the_statement(N, L, prec):
    """Plane waves (along x, along z, oblique) and a random field, R = 0 and 3: each of the six components within 1e-11 (fp64
    plan) / 1e-5 (f32 plan) of max|T| of the statement applied to the statement's own delta(k) uploaded as a half spectrum;
    once through the device's own r2c; the oblique wave against its closed form; the trace."""
    box, dt = _box(prec, N, L), DT[prec]
    for R in wc.SMOOTHINGS:
        for name, delta in sorted(_densities(N, L).items()):
            dk = wn.rfftn(wn.stored(delta, dt), dt)
            want = wn.tidal_tensor_k(dk, L, R, dt)
            T = web.tidal_tensor(box, delta_k=_upload_half(box.engine, dk), smoothing=R)
            assert isinstance(T, web.TensorField) and (T.kind, T.smoothing) == ("tidal", R)
            assert all(isinstance(c, DeviceArray) and c.kind == REAL for c in T.components) and T.xy is T.components[3]
            got = _host(T)
            scale = np.max(np.abs(want))
            err = np.max(np.abs(got - want), axis=(1, 2, 3)) / scale
            print("%s, R = %g, %s, N = %d, L = %s: max error per component %s of max|T| = %.3e"
                  % (name, R, prec, N, L, " ".join("%.2e" % e for e in err), scale))
            assert scale > 1e-3 and np.all(err <= TENSOR_TOL[prec])
            if name == "oblique":
                wave, _, _ = wc.plane_wave_tidal(N, L, wc.WAVES[name], R)
                assert np.max(np.abs(got - wave)) <= TENSOR_TOL[prec] * scale
        T = box.tidal_tensor(delta, smoothing=R)             # the random field, r2c on the device
        got = _host(T)
        err = np.max(np.abs(got - want)) / scale
        print("random through r2c, R = %g, %s: max error %.3e" % (R, prec, err))
        assert err <= TENSOR_TOL[prec]
        assert np.max(np.abs(np.asarray(T.trace()) - (got[0] + got[1] + got[2]))) <= 4 * np.finfo(dt).eps * scale


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_nyquist_rules(N, L, prec):
    """A single mode on each Nyquist plane: the off-diagonal components that touch the axis are exactly 0, the diagonal is
    not; a k = 0 spike gives zeros."""
    box = _box(prec, N, L)
    for axis in range(3):
        spec, _ = wc.nyquist_mode_spectrum(N, axis)
        T = _host(web.tidal_tensor(box, delta_k=_upload_half(box.engine, spec), smoothing=1.5))
        for q, (i, j) in enumerate(wn.PAIRS):
            if i == j:
                assert np.max(np.abs(T[q])) > 0.
            elif axis in (i, j):
                assert np.all(T[q] == 0.)
    spec = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    spec[0, 0, 0] = 5.
    assert np.all(_host(web.tidal_tensor(box, delta_k=_upload_half(box.engine, spec))) == 0.)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_shear_tensor(N, L, prec):
    """The velocity of realise_velocity for a field without power on the Nyquist planes: Sigma_ij = (f H a / H0) T_ij; the same
    for the statement's linear velocity; a velocity that is no gradient: the statement.  All to the tensor tolerances.

    realise_velocity keeps the reference's mode numbering, which at N = 18 gives the indices 7 and 11 the mode 0
    (hostgeom.mode_numbers): there it is not the linear velocity, so the field given to it has no power on those planes
    either.  The statement's own linear velocity has no such planes and is held to the identity on every other mode."""
    box, dt = _box(prec, N, L), DT[prec]
    dk = wn.rfftn(wn.stored(wc.random_field(N), dt), dt)
    h = N // 2
    dk[h, :, :] = 0.
    dk[:, h, :] = 0.
    dk[:, :, h] = 0.
    a = 1. / (1. + box.redshift)
    fac = 100. * box.cosmo['h'] * fb_box._ccl.h_over_h0(box.cosmo, a=a) * fb_box._ccl.growth_rate(box.cosmo, a=a) * a
    H0 = 100. * box.cosmo['h']
    exact = [np.fft.irfftn(v, s=(N, N, N), axes=(0, 1, 2)) for v in wn.linear_velocity_k(dk.astype(np.complex128), L, fac)]
    dq = dk.copy()
    for idx in np.nonzero(hostgeom.mode_numbers(N) != np.fft.fftfreq(N, 1. / N))[0]:
        dq[idx, :, :] = 0.
        dq[:, idx, :] = 0.
        if idx <= h:
            dq[:, :, idx] = 0.
    vk = box.realise_velocity(delta_k=_upload_half(box.engine, dq), inplace=False)
    vel = [box.to_real(v) for v in vk]
    for R in wc.SMOOTHINGS:
        for name, v, spec in (("realise_velocity", vel, dq), ("the statement's linear velocity", exact, dk)):
            S = web.shear_tensor(box, v, smoothing=R)
            assert (S.kind, S.smoothing) == ("shear", R)
            want = (fac / H0) * wn.tidal_tensor_k(spec, L, R, dt)
            scale = np.max(np.abs(want))
            err = np.max(np.abs(_host(S) - want)) / scale
            print("%s, R = %g, %s, N = %d, L = %s: max error %.3e of max|Sigma| = %.3e" % (name, R, prec, N, L, err, scale))
            assert scale > 1e-4 and err <= TENSOR_TOL[prec]
        v = wc.rotational_velocity(N, L)
        want = wn.shear_tensor(v, L, R, 70., dt)
        scale = np.max(np.abs(want))
        err = np.max(np.abs(_host(web.shear_tensor(box, v, smoothing=R, H0=70.)) - want)) / scale
        print("rotational velocity, R = %g, %s: max error %.3e of max|Sigma| = %.3e" % (R, prec, err, scale))
        assert scale > 1e-3 and err <= TENSOR_TOL[prec]
    cw = box.cosmic_web(kind="shear", velocity=v, smoothing=3., H0=70., threshold=0.)         # H0 reaches the tensor
    ref = web.classify(web.shear_tensor(box, v, smoothing=3., H0=70.), threshold=0.)
    np.testing.assert_array_equal(cw.counts, ref.counts)
    np.testing.assert_array_equal(cw.classes.host(), ref.classes.host())


def test_the_k_space_kernels_refuse_aliasing():
    N, L = GEOMS[0]
    eng = _box("f32", N, L).engine
    bufs = [eng.empty(HALF) for _ in range(7)]
    for outs in (bufs[:6], bufs[1:6] + [bufs[1]]):            # an output that is the input; two outputs that are one buffer
        with pytest.raises(_lib.FastBoxError, match="distinct"):
            _lib.call("fb_tidal_k", eng._plan, bufs[0].ptr, web._ptrs(outs), 0., eng.stream)
    with pytest.raises(_lib.FastBoxError, match="distinct"):                  # bufs[2] is the third input
        _lib.call("fb_shear_k", eng._plan, web._ptrs(bufs[:3]), web._ptrs(bufs[2:] + [eng.empty(HALF)]), 0., 70., eng.stream)


# ---- eigenvalues, isolated from the FFT -----------------------------------------------------------------------------------------
def _eigen_cases(N, L, prec):
    comp, _ = wc.exact_cube(N)
    return {"constructed": comp, "random-field tensor": _random_tensor(N, L, prec)[0]}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", EIGEN_GEOMS, ids=EIGEN_IDS)
def test_eigenvalues_are_backward_stable(N, L, prec):
    """Uploaded component cubes -- diagonal matrices of small integers in every order, the same turned by the 3-4-5 rotation
    about each axis, diag(1, 1, 1), diag(2, 1, 1), rank one, zero, scalings by 1e+-6, and the tensor of the random field --
    against np.linalg.eigvalsh of the components as downloaded: |error| <= 1024 * 2^-53 * ||A||_F per voxel (plus 2^-24 |lambda|
    for the store on f32 plans); descending order and lambda_1 + lambda_2 + lambda_3 = trace to the same bound.

    Measured on an MI355X: at most 12.1 x 2^-53 ||A||_F on the random-field tensors (30^3, f64) and 3.6 on the constructed
    matrices; on f32 plans at most 1.8 beyond the store (cosmic web)."""
    box = _box(prec, N, L)
    for name, comp in sorted(_eigen_cases(N, L, prec).items()):
        T = web.tensor_field(box, list(comp))
        down = _host(T)
        np.testing.assert_array_equal(down, wn.stored(comp, DT[prec]))
        lam = web.eigenvalues(T)
        assert len(lam) == 3 and all(isinstance(e, DeviceArray) and e.kind == REAL for e in lam)
        got = np.array([np.asarray(e) for e in lam])
        want = wn.eigenvalues(down)
        bound = wn.eigen_bound(down)
        store = 2. ** -24 * np.abs(want) if prec == "f32" else np.zeros_like(want)
        fro = np.where(bound > 0., bound / 1024., 1.)
        print("%s, %s, N = %d: max |error| %.1f x 2^-53 ||A||_F (bound 1024)%s" % (
            name, prec, N, np.max(np.maximum(np.abs(got - want) - store, 0.) / fro), " beyond the f32 store" if prec == "f32" else ""))
        assert np.all(np.abs(got - want) <= bound + store)
        assert np.all(got[0] >= got[1]) and np.all(got[1] >= got[2])
        assert np.all(np.abs(got.sum(axis=0) - (down[0] + down[1] + down[2])) <= bound + store.sum(axis=0))


# ---- classes and counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", EIGEN_GEOMS, ids=EIGEN_IDS)
def test_classes_of_constructed_matrices_are_literal(N, L, prec):
    box = _box(prec, N, L)
    comp, lam = wc.exact_cube(N)
    want = np.sum(lam > wc.INT_THRESHOLD, axis=0).astype(np.uint8)
    cw = web.classify(web.tensor_field(box, list(comp)), threshold=wc.INT_THRESHOLD)
    assert isinstance(cw, web.CosmicWeb) and isinstance(cw.classes, web.ClassCube) and cw.eigenvalues is None
    np.testing.assert_array_equal(cw.classes.host(), want)
    assert cw.counts.dtype == np.int64 and cw.counts.shape == (1, 4) and cw.n_nan == 0 and cw.weight_sums is None
    np.testing.assert_array_equal(cw.counts[0], np.bincount(want.ravel(), minlength=4))
    np.testing.assert_array_equal(cw.volume_fraction, cw.counts / float(N) ** 3)
    for kind, name in enumerate(web.CLASS_NAMES):
        m = cw.mask(name)
        assert isinstance(m, DeviceArray) and m.kind == REAL
        np.testing.assert_array_equal(np.asarray(m), (want == kind).astype(np.float64))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_classes_of_the_oblique_wave_are_literal(N, L, prec):
    """lambda = (s delta, 0, 0) sorted, threshold 0.3 s A: a sheet where delta > 0.3 A, a void elsewhere."""
    box = _box(prec, N, L)
    for R in wc.SMOOTHINGS:
        _, delta, s = wc.plane_wave_tidal(N, L, wc.WAVES["oblique"], R)
        thr = 0.3 * s * wc.AMPLITUDE
        assert np.min(np.abs(s * delta - thr)) > 1e-3 * s * wc.AMPLITUDE          # no value near the threshold
        want = (s * delta > thr).astype(np.uint8)
        cw = box.cosmic_web(delta, smoothing=R, threshold=thr)
        np.testing.assert_array_equal(cw.classes.host(), want)
        np.testing.assert_array_equal(cw.counts, [[np.sum(want == 0), np.sum(want == 1), 0, 0]])


def _scan(prec, N, L, nt):
    lam = wn.eigenvalues(_random_tensor(N, L, prec)[0])
    sigma = float(np.std(lam))
    return {1: np.array([0.]), 2: np.array([0., 0.2 * sigma]), 16: sigma * 0.1 * np.arange(-5, 11)}[nt]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nt", (1, 2, 16))
@pytest.mark.parametrize("N,L", EIGEN_GEOMS, ids=EIGEN_IDS)
def test_classes_counts_and_weight_sums_of_the_random_tensor(N, L, nt, prec):
    """For every threshold of the scan, with each class_at: the class cube is the statement's on the downloaded tensor except
    where a numpy eigenvalue lies within the eigenvalue bound of the threshold (at most 1e-3 of the voxels); counts are
    bincount of the device's own class cube, exactly; weight sums are the fp64 numpy sums over the device's classes to 1e-12;
    two calls are bitwise equal; every nullable output left out leaves the others as they were."""
    box, dt = _box(prec, N, L), DT[prec]
    comp, delta = _random_tensor(N, L, prec)
    thr = _scan(prec, N, L, nt)
    T = web.tensor_field(box, list(comp))
    wh = wn.stored(1. + delta, dt)
    w = box.engine.upload(wh, REAL)
    lam = wn.eigenvalues(_host(T))
    bound = wn.eigen_bound(_host(T))
    full = None
    for j in range(nt):
        eig, classes, counts, wsum, n_nan = web._eigen(T, thr, j, w, True, True, True)
        cls = classes.host()
        near = np.any(np.abs(lam - thr[j]) <= bound, axis=0)
        assert np.mean(near) <= 1e-3
        np.testing.assert_array_equal(cls[~near], wn.classify(lam, thr[j])[~near])
        assert n_nan == 0 and counts.shape == (nt, 4) and np.all(counts.sum(axis=1) == N ** 3)
        np.testing.assert_array_equal(counts[j], np.bincount(cls.ravel(), minlength=4))
        ref = np.array([np.sum(wh[cls == c], dtype=np.float64) for c in range(4)])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(ref != 0., np.abs(wsum[j] - ref) / np.abs(ref), np.abs(wsum[j]))
        print("%s, N = %d, nt = %d, class_at %d: weight sums within %.2e relative of the fp64 numpy sums" % (prec, N, nt, j, np.max(rel)))
        np.testing.assert_allclose(wsum[j], ref, rtol=1e-12, atol=0.)
        eig = np.array([np.asarray(e) for e in eig])
        if full is None:
            full = (eig, counts, wsum)
        np.testing.assert_array_equal(eig, full[0])            # class_at changes the class cube only
        np.testing.assert_array_equal(counts, full[1])
        np.testing.assert_array_equal(wsum, full[2])
    eig0, counts0, wsum0 = full
    cls0 = web._eigen(T, thr, 0, w, False, True, False)[1].host()                        # classes alone
    np.testing.assert_array_equal(cls0, web._eigen(T, thr, 0, w, True, True, True)[1].host())
    e1 = web._eigen(T, thr, 0, None, True, False, False)[0]                              # eigenvalues alone
    np.testing.assert_array_equal(np.array([np.asarray(e) for e in e1]), eig0)
    _, none, c2, w2, _ = web._eigen(T, thr, 0, w, False, False, True)                    # counts and sums alone
    assert none is None
    np.testing.assert_array_equal(c2, counts0)
    np.testing.assert_array_equal(w2, wsum0)
    _, _, c3, w3, _ = web._eigen(T, thr, 0, None, False, False, True)                    # no weight
    assert w3 is None
    np.testing.assert_array_equal(c3, counts0)
    cw = web.classify(T, threshold=thr if nt > 1 else thr[0], weight=w, return_eigenvalues=True)
    np.testing.assert_array_equal(cw.counts, counts0)
    np.testing.assert_array_equal(cw.weight_sums, wsum0)
    np.testing.assert_allclose(cw.mass_fraction.sum(axis=1), 1., rtol=0, atol=1e-14)
    assert (cw.classes is None) == (nt > 1) and len(cw.eigenvalues) == 3
    if nt > 1:
        with pytest.raises(ValueError, match="classes"):
            cw.mask("void")


# ---- NaN and inf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", EIGEN_GEOMS, ids=EIGEN_IDS)
def test_nan_and_inf_components(N, L, prec):
    """A few NaN and +-inf components: class 255 and NaN eigenvalues there, n_nan exact, every other voxel unchanged -- and the
    call returns: the solver's sweeps do not depend on the data."""
    box = _box(prec, N, L)
    comp, _ = _random_tensor(N, L, prec)
    bad, vox = wc.poisoned(comp)
    clean = web.classify(web.tensor_field(box, list(comp)), threshold=0., return_eigenvalues=True)
    cw = web.classify(web.tensor_field(box, list(bad)), threshold=0., return_eigenvalues=True)
    hit = np.zeros(N ** 3, dtype=bool)
    hit[vox] = True
    cls, ref = cw.classes.host().ravel(), clean.classes.host().ravel()
    assert cw.n_nan == vox.size and clean.n_nan == 0
    assert np.all(cls[hit] == web.NAN_CLASS)
    np.testing.assert_array_equal(cls[~hit], ref[~hit])
    np.testing.assert_array_equal(cw.counts[0], np.bincount(cls[~hit], minlength=4))
    for e, r in zip(cw.eigenvalues, clean.eigenvalues):
        e, r = np.asarray(e).ravel(), np.asarray(r).ravel()
        assert np.all(np.isnan(e[hit])) and not np.any(np.isnan(e[~hit]))
        np.testing.assert_array_equal(e[~hit], r[~hit])
    assert np.sum(cw.counts) + cw.n_nan == N ** 3
    if prec == "f64":                                    # finite components whose differences overflow in the solve: counted as NaN
        huge = np.array(comp)
        huge[:, 1, 2, 3] = (1.7e308, -1.7e308, 1.7e308, 1.7e308, -1.7e308, 1.7e308)
        ov = web.classify(web.tensor_field(box, list(huge)), threshold=0., return_eigenvalues=True)
        at = ov.classes.host()[1, 2, 3], [np.asarray(e)[1, 2, 3] for e in ov.eigenvalues]
        assert (ov.n_nan == 1 and at[0] == web.NAN_CLASS and np.all(np.isnan(at[1]))) or (ov.n_nan == 0 and np.all(np.isfinite(at[1])))
        assert np.sum(ov.counts) + ov.n_nan == N ** 3


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_cosmic_web_end_to_end(prec):
    """A realised 32^3 log-normal box: the fractions sum to 1, the mean delta rises from void to knot, the masks are fields."""
    box = CosmoBox(cosmo=default_cosmo, box_scale=(128., 128., 128.), nsamp=32, realise_now=False, precision=prec, rng="device",
                   seed=17)
    delta = box.lognormal(box.realise_density())
    cw = box.cosmic_web(delta, smoothing=4., threshold=0., weight=1. + delta)
    assert cw.n_nan == 0 and np.sum(cw.counts) == 32 ** 3 and np.all(cw.counts > 0)
    np.testing.assert_allclose(cw.volume_fraction.sum(), 1., rtol=0, atol=1e-15)
    np.testing.assert_allclose(cw.mass_fraction.sum(), 1., rtol=0, atol=1e-14)
    mean_delta = cw.weight_sums[0] / cw.counts[0] - 1.
    print("%s: volume fractions %s, mass fractions %s, mean delta per class %s" % (prec, np.round(cw.volume_fraction[0], 4),
                                                                                   np.round(cw.mass_fraction[0], 4), np.round(mean_delta, 4)))
    assert np.all(np.diff(mean_delta) > 0.)
    cls = cw.classes.host()
    for kind in range(4):
        m = cw.mask(kind)
        np.testing.assert_array_equal(np.asarray(m), (cls == kind).astype(np.float64))
        k, pk, modes = box.power_spectrum(m)
        assert np.all(np.isfinite(pk[modes > 0])) and np.any(pk > 0.)
    same = box.cosmic_web(delta, smoothing=4., threshold=0., weight=1. + delta)
    np.testing.assert_array_equal(same.counts, cw.counts)
    np.testing.assert_array_equal(same.weight_sums, cw.weight_sums)
    scan = box.cosmic_web(delta, smoothing=4., threshold=np.linspace(0., 0.6, 4))
    np.testing.assert_array_equal(scan.counts[0], cw.counts[0])
    assert np.all(np.diff(scan.counts[:, 0]) >= 0) and np.all(np.diff(scan.counts[:, 3]) <= 0)      # more voids, fewer knots


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(monkeypatch):
    N, L = GEOMS[1]
    box, other = _box("f32", N, L), _box("f64", N, L)
    eng = box.engine
    zero = np.zeros((N, N, N))
    T = web.tensor_field(box, [zero] * 6)
    foreign, spectrum, real = other.engine.upload(zero, REAL), eng.empty(HALF), eng.upload(zero, REAL)
    foreign_spectrum = other.engine.empty(HALF)
    other.engine.sync()
    real_bytes, half_bytes = web.field_bytes(N, "f32")
    assert (real_bytes, half_bytes) == (eng.nbytes[REAL], eng.nbytes[HALF])
    assert eng.free_bytes() > web.web_device_bytes(N, "f32", kind="shear", eigenvalues=True) > 0
    made = web.classify(T)
    eng.sync()

    def no_device(name, *args):
        raise AssertionError("device call %s before the arguments were checked" % name)
    monkeypatch.setattr(_lib, "call", no_device)
    for kw in (dict(delta_x=np.zeros((N, N, N + 1))), dict(delta_x=np.zeros((N, N))), dict(delta_x=foreign),
               dict(delta_x=zero, delta_k=spectrum), dict(delta_x=zero, smoothing=-1.), dict(delta_x=zero, smoothing=np.nan),
               dict(delta_k=np.zeros((N, N), dtype=complex)), dict(delta_k=foreign_spectrum)):
        with pytest.raises(ValueError):
            box.tidal_tensor(**kw)
    for kw in (dict(delta_x=zero.astype(complex)), dict(delta_x=spectrum), dict(delta_k=real)):
        with pytest.raises(TypeError):
            box.tidal_tensor(**kw)
    for vel in ([zero] * 2, [zero] * 4, [zero, zero, np.zeros((N, N))], [zero, zero, foreign]):
        with pytest.raises(ValueError, match="velocity"):
            web.shear_tensor(box, vel)
    with pytest.raises(TypeError, match="velocity"):
        web.shear_tensor(box, [zero, zero, spectrum])
    with pytest.raises(TypeError, match="velocity"):
        web.shear_tensor(box, 3.)
    for kw, name in ((dict(smoothing=-2.), "smoothing"), (dict(H0=0.), "H0"), (dict(H0=np.inf), "H0")):
        with pytest.raises(ValueError, match=name):
            web.shear_tensor(box, [zero] * 3, **kw)
    for bad in ([0.5, 0.], [0., 0.], [0., np.nan], [np.inf], np.arange(17.), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="threshold"):
            web.classify(T, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            box.cosmic_web(zero, threshold=bad)
    with pytest.raises(TypeError, match="tensor"):
        web.classify([zero] * 6)
    with pytest.raises(TypeError, match="tensor"):
        web.eigenvalues(real)
    with pytest.raises(ValueError, match="weight"):
        web.classify(T, weight=np.zeros((N, N)))
    with pytest.raises(ValueError, match="weight"):
        web.classify(T, weight=foreign)
    with pytest.raises(ValueError, match="weight"):
        box.cosmic_web(zero, weight=np.zeros(3))
    with pytest.raises(TypeError, match="weight"):
        web.classify(T, weight=spectrum)
    for kw, name in ((dict(kind="density"), "kind"), (dict(kind="shear"), "velocity"), (dict(velocity=[zero] * 3), "velocity"),
                     (dict(kind="shear", velocity=[zero] * 3, delta_x=zero), "delta_x"), (dict(delta_x=zero, H0=70.), "H0"),
                     (dict(kind="shear", velocity=[zero] * 3, H0=-1.), "H0")):
        with pytest.raises(ValueError, match=name):
            box.cosmic_web(**kw)
    with pytest.raises(ValueError, match="components"):
        web.tensor_field(box, [zero] * 5)
    with pytest.raises(ValueError, match="components"):
        web.tensor_field(box, [zero] * 5 + [foreign])
    monkeypatch.setattr(eng, "free_bytes", lambda: 1 << 10)
    with pytest.raises(MemoryError, match="work memory"):
        box.tidal_tensor(zero)
    with pytest.raises(MemoryError, match="work memory"):
        web.shear_tensor(box, [real] * 3)
    with pytest.raises(MemoryError, match="work memory"):
        web.classify(T)
    with pytest.raises(MemoryError, match="work memory"):
        web.eigenvalues(T)
    with pytest.raises(MemoryError, match="work memory"):
        made.mask("void")
