"""GPU: the interferometer kernels (fb_uv_coverage, fb_uv_channel_sums, fb_uv_weight) through the C entries and
Interferometer.observe / psf / noise, against the numpy statement of tests/interferometer_numpy.py on the constructed cases of
tests/interferometer_cases.py, on both plan precisions.

The counts and their sums are integers: the device must give the statement's values exactly, and the same bits on every call.
fb_uv_weight forms its factor in fp64 and rounds once: bit-equal to the statement on the fp64 plan, equal to its single-rounding
form on the f32 plan.  The transformed cubes follow the project's parity tolerance for transformed fields: 1e-11 (fp64 plan) and
1e-5 (f32 plan) of the largest magnitude of the statement's result."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, DeviceArray, Interferometer, default_cosmo, _lib
from fastbox_amd import interferometer as itf
from fastbox_amd.sky import sky_draw_seed
from tests import interferometer_cases as ic
from tests import interferometer_numpy as inp

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
TOL = {"f64": 1e-11, "f32": 1e-5}
OBSERVE_GEOMS = ("n16", "n18", "cuboid")
OBSERVE_CASES = ("random1000", "random65-mult", "band-edge")


@functools.lru_cache(maxsize=None)
def _box(geom, prec, rng="numpy"):
    N, scale = ic.GEOMETRIES[geom]
    return CosmoBox(cosmo=default_cosmo, box_scale=scale, nsamp=N, redshift=ic.REDSHIFT, realise_now=False, precision=prec,
                    rng=rng, seed=21)


@functools.lru_cache(maxsize=None)
def _cases(geom):
    """name -> (samples, mult, the statement's counts), on the geometry's own tables; computed once, read-only."""
    N, sx, sy = ic.tables(geom)
    out = {}
    for name, samples, mult in ic.cases(N, sx, sy):
        S = inp.coverage(N, samples, mult, sx, sy)
        S.setflags(write=False)
        out[name] = (samples, mult, S)
    return out


def _dl(eng, ptr, shape, dtype):
    h = np.empty(shape, dtype=dtype)
    _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), ptr, h.nbytes, eng.stream)
    eng.sync()
    return h


def _coverage(eng, samples, mult, sx, sy, counts_buf, accumulate):
    samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 2)
    ns = samples.shape[0]
    keep = [eng.upload_raw(samples) if ns else None, eng.upload_raw(np.ascontiguousarray(mult, dtype=np.int32)) if mult is not None else None,
            eng.upload_raw(np.ascontiguousarray(sx)), eng.upload_raw(np.ascontiguousarray(sy))]
    _lib.call("fb_uv_coverage", eng._plan, keep[0].ptr if keep[0] else None, keep[1].ptr if keep[1] else None, ns, keep[2].ptr,
              keep[3].ptr, counts_buf.ptr, accumulate, eng.stream)
    eng.sync()
    N = eng.N
    return _dl(eng, counts_buf.ptr, (N, N, N), np.int32)


def _garbage_counts(eng):
    return eng.upload_raw(np.full(eng.N ** 3, 0x5a5a5a5a, dtype=np.int32))


def _sums(eng, counts_buf):
    out = eng.upload_raw(np.full(2 * eng.N, -77, dtype=np.int64))
    _lib.call("fb_uv_channel_sums", eng._plan, counts_buf.ptr, out.ptr, eng.stream)
    return _dl(eng, out.ptr, (2, eng.N), np.int64)


def _same(what, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d differ, first at %s: device %r, expected %r" % (what, len(bad), got.size, i, got[i], want[i]))


def _close(what, got, want, prec):
    scale = float(np.max(np.abs(want)))
    dev = float(np.max(np.abs(np.asarray(got) - want)))
    print("%s [%s]: deviation %.3e of max %.3e (bound %.0e)" % (what, prec, dev, scale, TOL[prec]))
    assert dev <= TOL[prec] * scale, "%s [%s]: deviation %.3e, max |statement| %.3e" % (what, prec, dev, scale)


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(ic.GEOMETRIES))
def test_channel_tables_are_the_boxs_own(geom):
    N, sx, sy = ic.tables(geom)
    bx, by = itf.channel_scales(_box(geom, "f64"))
    assert np.array_equal(bx, sx) and np.array_equal(by, sy)


# ---- fb_uv_coverage, fb_uv_channel_sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", sorted(ic.GEOMETRIES))
def test_coverage_and_sums_are_exact(geom, prec):
    N, sx, sy = ic.tables(geom)
    eng = _box(geom, prec).engine
    for name, (samples, mult, S) in _cases(geom).items():
        buf = _garbage_counts(eng)                                            # accumulate = 0 clears it
        got = _coverage(eng, samples, mult, sx, sy, buf, 0)
        _same("%s counts" % name, got, S)
        _same("%s sums" % name, _sums(eng, buf), np.stack(inp.channel_sums(S)))
        again = _coverage(eng, samples, mult, sx, sy, _garbage_counts(eng), 0)
        _same("%s second call" % name, again, got)
        twice = _coverage(eng, samples, mult, sx, sy, buf, 1)                 # on top of the first
        _same("%s accumulated" % name, twice, 2 * S)
        _same("%s accumulated (statement)" % name, twice, inp.coverage(N, samples, mult, sx, sy, counts=S))
        _same("%s sums of the doubled counts" % name, _sums(eng, buf), np.stack(inp.channel_sums(2 * S)))
    a, b = _cases(geom)["copies-expanded"][2], _cases(geom)["copies-collapsed"][2]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", ("n16", "n18"))
def test_coverage_on_hand_made_tables(geom, prec):
    eng = _box(geom, prec).engine
    N = eng.N
    for what, (sx, sy), samples in (("edge", ic.edge_tables(N), ic.edge_set(N)),
                                    ("upper-empty", ic.upper_empty_tables(N), ic.upper_empty_set(N))):
        S = inp.coverage(N, samples, None, sx, sy)
        buf = _garbage_counts(eng)
        _same(what, _coverage(eng, samples, None, sx, sy, buf, 0), S)
        sums = _sums(eng, buf)
        _same(what + " sums", sums, np.stack(inp.channel_sums(S)))
        if what == "upper-empty":
            assert np.all(sums[:, N // 2:] == 0) and np.all(sums[0, :N // 2] == 100)
    # ties go to even; +-N/2 is accepted and folds onto row N/2; the next one out is rejected
    sx, sy = ic.edge_tables(N)
    one = lambda bx, by: _coverage(eng, [[bx, by]], None, sx, sy, _garbage_counts(eng), 0)[:, :, N - 1]
    assert one(1., 0.)[0, 0] == 2 and one(3., 0.)[2, 0] == 1 and one(5., 0.)[2, 0] == 1 and one(-3., 0.)[N - 2, 0] == 1
    assert one(float(N), 0.)[N // 2, 0] == 2 and one(0., -float(N))[0, N // 2] == 2
    assert one(N + 2., 0.).sum() == 0 and one(N + 1., 0.).sum() == (2 if (N // 2) % 2 == 0 else 0)


# ---- fb_uv_weight ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", ("n16", "n18"))
def test_weight_rounds_once(geom, prec):
    box = _box(geom, prec)
    eng, N = box.engine, box.N
    S = _cases(geom)["random1000"][2]
    assert (S == 0).any() and (S > 1).any()
    spec = np.fft.fft2(ic.smooth_cube(N), axes=(0, 1)).astype(eng.cdtype)                 # the statement's own spectrum
    rs = np.random.RandomState(4)
    scale = rs.uniform(0.05, 3., N)
    scale[3] = 0.
    counts = eng.upload_raw(np.ascontiguousarray(S))
    scale_dev = eng.upload_raw(scale)
    for mode in (inp.NATURAL, inp.UNIFORM, inp.SQRT):
        cube = eng.upload(spec, "full")
        _lib.call("fb_uv_weight", eng._plan, cube.ptr, counts.ptr, mode, scale_dev.ptr, eng.stream)
        got = _dl(eng, cube.ptr, (N, N, N), eng.cdtype)
        want = inp.weight(spec, S, mode, scale)
        _same("mode %d real" % mode, got.real, want.real)
        _same("mode %d imag" % mode, got.imag, want.imag)
        assert not got[:, :, 3].any() and got.any()
    cube = eng.upload(spec, "full")
    with pytest.raises(_lib.FastBoxError):
        _lib.call("fb_uv_weight", eng._plan, cube.ptr, counts.ptr, 3, scale_dev.ptr, eng.stream)


# ---- observe, psf, noise ------------------------------------------------------------------------------------------------------------
def _instrument(geom, prec, name, rng="numpy"):
    samples, mult, S = _cases(geom)[name]
    return Interferometer(_box(geom, prec, rng), baselines=samples, multiplicity=mult), S


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", OBSERVE_GEOMS)
def test_observe_psf_and_noise_match_the_statement(geom, prec):
    box = _box(geom, prec)
    N = box.N
    cube = ic.smooth_cube(N)
    beam = np.exp(-0.5 * (np.arange(N) - N / 2.) ** 2 / (0.3 * N) ** 2)[:, None, None] * np.ones((N, N, N))
    sigma = np.linspace(0.5, 2., N)
    for name in OBSERVE_CASES:
        inst, S = _instrument(geom, prec, name)
        cov = inst.uv_coverage()
        assert cov is inst.uv_coverage()
        tot, ncell = inp.channel_sums(S)
        _same(name + " counts", cov.counts.host(), S)
        _same(name + " tot", cov.tot, tot)
        _same(name + " ncell", cov.ncell, ncell)
        assert np.array_equal(cov.empty_channels, np.flatnonzero(tot == 0)) and (cov.du, cov.dv) == itf.uv_cell(box)
        assert cov.n_samples == (len(_cases(geom)[name][0]) if _cases(geom)[name][1] is None else _cases(geom)[name][1].sum())
        empty = tot == 0
        assert empty.any() == (name == "band-edge")
        for weighting in ("natural", "uniform"):
            obs = inst.observe(cube, weighting=weighting, return_psf=True)
            assert isinstance(obs.dirty, DeviceArray) and obs.dirty.kind == "real" and obs.noise is None and obs.coverage is cov
            want = inp.observe(cube, S, weighting)
            _close("%s %s dirty" % (name, weighting), obs.dirty.host(), want.real, prec)
            _close("%s %s psf" % (name, weighting), obs.psf.host(), inp.psf(S, weighting).real, prec)
            assert np.allclose(obs.psf.host()[0, 0, ~empty], 1., rtol=0, atol=TOL[prec])
            assert not obs.dirty.host()[:, :, empty].any() and not obs.psf.host()[:, :, empty].any()
            _same("psf on its own", inst.psf(weighting).host(), obs.psf.host())
            withbeam = inst.observe(cube, weighting=weighting, primary_beam=beam)
            _close("%s %s dirty with a beam" % (name, weighting), withbeam.dirty.host(), inp.observe(cube, S, weighting, beam=beam).real, prec)
        # noise: the same g as the statement's through the legacy stream
        np.random.seed(5)
        obs = inst.observe(cube, sigma=sigma)
        np.random.seed(5)
        g = np.random.normal(0., 1., (N, N, N))
        nwant = inp.noise(g, S, sigma).real
        _close(name + " noise", obs.noise.host(), nwant, prec)
        _close(name + " dirty + noise", obs.dirty.host(), inp.observe(cube, S, "natural").real + nwant, prec)
        assert not obs.noise.host()[:, :, empty].any() and not obs.dirty.host()[:, :, empty].any()
        np.random.seed(5)
        _same("noise on its own", inst.noise(sigma).host(), obs.noise.host())
        np.random.seed(5)
        _close(name + " scalar sigma", inst.noise(0.7).host(), inp.noise(g, S, 0.7).real, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", OBSERVE_GEOMS)
def test_uniform_weighting_of_full_coverage_is_the_identity(geom, prec):
    inst, S = _instrument(geom, prec, "everywhere")
    assert S.min() >= 1
    cube = ic.smooth_cube(inst.box.N)
    obs = inst.observe(cube, weighting="uniform")
    assert obs.coverage.empty_channels.size == 0
    _close("identity", obs.dirty.host(), cube, prec)
    _close("identity against the statement", obs.dirty.host(), inp.observe(cube, S, "uniform").real, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_device_and_host_inputs_give_the_same_bits(prec):
    inst, S = _instrument("n18", prec, "random1000")
    box = inst.box
    cube = ic.smooth_cube(box.N)
    dev = box.engine.upload(cube, "real")
    a = inst.observe(cube, weighting="uniform").dirty.host()
    b = inst.observe(dev, weighting="uniform").dirty.host()
    _same("device against host input", b, a)
    _same("the input cube is left alone", dev.host(), box.engine.upload(cube, "real").host())
    from fastbox_amd import BeamModel
    _same("unit beam model", inst.observe(dev, weighting="uniform", primary_beam=BeamModel(box)).dirty.host(), a)


@pytest.mark.parametrize("prec", PRECS)
def test_device_generator_noise(prec):
    """rng='device': g is fb_sky_noise_cube with sigma = 1 and the box's next sky seed."""
    inst, S = _instrument("n16", prec, "random1000", rng="device")
    box, eng = inst.box, inst.box.engine
    N = box.N
    draws = getattr(box, "_sky_draws", 0)
    got = inst.noise(1.3).host()
    assert box._sky_draws == draws + 1
    g, one = eng.empty("real"), np.ones(N)
    _lib.call("fb_sky_noise_cube", eng._plan, one.ctypes.data_as(_lib.P_double), None, sky_draw_seed(box.seed, draws + 1), g.ptr, eng.stream)
    eng.sync()
    _close("device noise", got, inp.noise(g.host(), S, 1.3).real, prec)
    assert not np.array_equal(inst.noise(1.3).host(), got)                               # the next seed


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_bad_arguments_raise_before_the_device_is_touched(prec, monkeypatch):
    box = _box("n16", prec)
    eng, N = box.engine, box.N
    samples = _cases("n16")["random65"][0]

    def no_alloc(nbytes):
        raise AssertionError("a device buffer was allocated")
    monkeypatch.setattr(eng, "_alloc_bytes", no_alloc)
    with pytest.raises(ValueError):
        Interferometer(box, baselines=[[1., np.nan]])
    with pytest.raises(ValueError):
        Interferometer(box, baselines=[[-np.inf, 1.]])
    with pytest.raises(ValueError):
        Interferometer(box, baselines=samples, multiplicity=np.full(len(samples), 2 ** 25))          # 2 x 65 x 2^25 > 2^31 - 1
    inst = Interferometer(box, baselines=samples)
    cube = ic.smooth_cube(N)
    for bad in (lambda: inst.observe(cube, weighting="briggs"), lambda: inst.psf("robust"), lambda: inst.noise(1., weighting="x"),
                lambda: inst.observe(cube, sigma=-1.), lambda: inst.noise(-0.5), lambda: inst.noise(np.full(N, -1.)),
                lambda: inst.noise(np.ones(N + 1)), lambda: inst.noise(np.nan),
                lambda: inst.observe(cube, weighting="uniform", sigma=1.),           # the noise cube is natural weighting only
                lambda: inst.observe(cube[:-1]), lambda: inst.observe(np.zeros((N, N))),
                lambda: inst.observe(cube, primary_beam=np.ones((N, N)))):
        with pytest.raises(ValueError):
            bad()
    # not enough memory: MemoryError, still before any allocation
    monkeypatch.setattr(eng, "free_bytes", lambda: 4 * N ** 3 + eng.nbytes["full"] - 1)
    for bad in (inst.uv_coverage, lambda: inst.observe(cube), inst.psf, lambda: inst.noise(1.)):
        with pytest.raises(MemoryError):
            bad()
    monkeypatch.undo()
    assert inst.observe(cube).dirty.host().shape == (N, N, N)
