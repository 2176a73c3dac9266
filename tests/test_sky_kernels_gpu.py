"""GPU: the sky and noise kernels (fb_field_kernels.h k_sky_*, driven from fastbox_amd/sky.py) against host statements
of the same operations (oracle/sky_oracle.py, tests/sky_numpy.py) and, for rng='device', against host models of the exact
draws of streams 2, 3 and 4 (fastbox_amd/rng.py).  Sizes: tests/sky_numpy.py SIZES -- 18 and 30 have N % 4 = 2, where a group
of four consecutive voxels of the noise cube straddles two lines of sight; 72 takes two trips of k_sky_fg_cube's block.

Single precision with the device generator: the hardware log2, sin and cos are not correctly rounded, so the bound is
taken from the host model itself -- delta_ref = max |f32 model - f64 model| on the same Philox words, and the device must lie
within 4 delta_ref of the f64 model (a couple of ulp in the hardware's transcendentals where numpy's are within one)."""
import numpy as np
import pytest
import scipy.ndimage

from oracle import sky_oracle as so
from tests import sky_numpy as sn

pytestmark = pytest.mark.gpu

PRECISIONS = [("f64", 1e-12), ("f32", 2e-6)]          # the tolerances of tests/test_sky_gpu.py
SEED = 4


def _box(N, precision, rng="numpy", box_scale=2e3, seed=SEED):
    from fastbox_amd import CosmoBox, default_cosmo
    return CosmoBox(cosmo=default_cosmo, box_scale=box_scale, nsamp=N, redshift=0.8, realise_now=False,
                    precision=precision, rng=rng, seed=seed)


def _sigma(box):
    ang_x, _ = box.pixel_array()
    return so.radiometer_sigma(box.freq_array(), ang_x, **sn.RADIOMETER)


def _fill_scratch(box, sigma):
    """An ordinary call that leaves 2 N large doubles in the plan's scratch (ratios near 1e3 and their log2, ~10): a
    read of a stale table entry is then a gross error."""
    from fastbox_amd import ForegroundModel
    freqs = box.freq_array()
    stale = np.concatenate([freqs / (freqs[0] / 1e3), np.log2(freqs / (freqs[0] / 1e3))])
    assert np.all(stale[box.N:box.N + 4] > 2 * sigma.max()) and np.all(stale[:box.N] > 2 * sigma.max())
    ForegroundModel(box).construct_cube(np.ones((box.N, box.N)), 0.0, freq_ref=freqs[0] / 1e3)
    box.engine.sync()


# ---- a. noise cube, host draws -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("N", sn.SIZES)
def test_noise_cube_numpy_draws_channel_by_channel(N, precision, tol):
    from fastbox_amd import NoiseModel
    box = _box(N, precision)
    sigma = _sigma(box)
    _fill_scratch(box, sigma)
    np.random.seed(31)
    cube = np.asarray(NoiseModel(box).realise_radiometer_noise(**sn.RADIOMETER))
    np.random.seed(31)
    want = so.radiometer_noise((N, N, N), sigma)
    assert cube.shape == (N, N, N)
    unit = sn.as_stored(np.random.RandomState(31).normal(0., 1., (N, N, N)), precision)
    ratio = cube / (unit * sigma[None, None, :])
    dev = np.max(np.abs(ratio - 1).reshape(-1, N), axis=0)
    assert np.all(dev < tol), "channels off: %s, worst |ratio - 1| %.3e" % (np.nonzero(dev >= tol)[0][:8], dev.max())
    assert np.max(np.abs(cube - want)) < tol * np.max(np.abs(want))


# ---- b. noise cube, device draws ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("N", sn.SIZES)
def test_noise_cube_device_draws_equal_the_host_model(N, precision):
    """Measured on the MI355X, f32, first draw (device deviation from the f64 model / delta_ref, in mK; sigma is 1e-3 to
    1e-2 mK): N = 16: 1.527e-09 / 1.518e-09, 18: 1.824e-08 / 1.824e-08, 24: 2.680e-08 / 2.680e-08, 30: 3.891e-08 /
    3.891e-08, 72: 1.505e-07 / 1.505e-07.  Both maxima sit on the element whose first uniform rounds towards 1 in float32
    (the radius sqrt(-2 ln u) is steep there), a rounding the device and the f32 model share."""
    from fastbox_amd import NoiseModel
    from fastbox_amd.sky import sky_draw_seed
    box = _box(N, precision, rng="device")
    sigma = _sigma(box)
    _fill_scratch(box, sigma)
    nm = NoiseModel(box)
    for draw in (1, 2):
        cube = np.asarray(nm.realise_radiometer_noise(**sn.RADIOMETER))
        seed = sky_draw_seed(SEED, draw)
        want = sn.noise_cube_model(N, seed, sigma, np.float64)
        dev = np.abs(cube - want)
        if precision == "f64":
            assert np.max(dev / np.abs(want)) < 1e-12, (draw, np.max(dev / np.abs(want)))
        else:
            delta_ref = np.max(np.abs(sn.noise_cube_model(N, seed, sigma, np.float32) - want))
            print("noise cube N=%d draw %d: device %.3e delta_ref %.3e" % (N, draw, dev.max(), delta_ref))
            assert np.isfinite(delta_ref) and delta_ref > 0
            assert dev.max() <= 4 * delta_ref, "draw %d: device deviation %.3e, delta_ref %.3e, worst channels %s" % (
                draw, dev.max(), delta_ref, np.argsort(dev.reshape(-1, N).max(axis=0))[-4:])


# ---- c. spectral-index map, device draws ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("N", sn.SIZES)
def test_spectral_index_device_draws_equal_the_host_model(N, precision):
    """mean + std * (stream 3), smoothed by the double loop of tests/sky_numpy.py.  Measured on the MI355X, f32 (device
    deviation from the f64 model / delta_ref, first draw): N = 16: 1.755e-07 / 1.755e-07, 18: 1.777e-07 / 1.777e-07,
    24: 1.819e-07 / 1.940e-07, 30: 1.969e-07 / 1.969e-07, 72: 1.992e-07 / 1.992e-07 (the storage of values near 2)."""
    from fastbox_amd import ForegroundModel
    from fastbox_amd.sky import sky_draw_seed
    mean, std = 2.07, 0.05
    box = _box(N, precision, rng="device")
    ang_x, _ = box.pixel_array()
    pix = ang_x[1] - ang_x[0]
    fg = ForegroundModel(box)
    for draw, sigma_pix in ((1, 1.5), (2, 0.6)):
        got = fg.realise_spectral_index(mean, std, smoothing_scale=sigma_pix * pix)
        w, r = so.gaussian_weights((sigma_pix * pix) / pix)          # the quotient sky.py forms
        seed = sky_draw_seed(SEED, draw)
        want = sn.wrap_smooth(sn.index_map_model(N, seed, mean, std, np.float64), w, r)
        dev = np.max(np.abs(got - want))
        if precision == "f64":
            assert dev < 1e-12 * np.max(np.abs(want)), (draw, dev)
        else:
            model32 = sn.wrap_smooth(sn.index_map_model(N, seed, mean, std, np.float32), w, r, "f32")
            delta_ref = np.max(np.abs(model32 - want))
            print("spectral index N=%d draw %d: device %.3e delta_ref %.3e" % (N, draw, dev, delta_ref))
            assert np.isfinite(delta_ref) and delta_ref > 0
            assert dev <= 4 * delta_ref, "draw %d: device deviation %.3e, delta_ref %.3e" % (draw, dev, delta_ref)


# ---- d. foreground amplitude map, device draws ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("box_scale", [2e3, sn.CUBOID], ids=["cubic", "cuboid"])
@pytest.mark.parametrize("N", sn.SIZES)
def test_foreground_map_device_draws_equal_the_host_model(N, box_scale, precision):
    """The oracle's map from the host model of stream 2, with and without smoothing.  f64: the bound of
    tests/test_sky_gpu.py.  f32: 4 delta_ref, with delta_ref the oracle on the f32 model of the noise against the oracle
    on the f64 model, plus the arithmetic of an f32 plan, which the oracle (float64 throughout) does not have: the map is a
    sum of N^2 products formed in log2(N^2) butterfly stages, for which a max error of ~ 2^-24 sqrt(log2 N^2) sqrt(2 ln N^2)
    rms is expected; 8 * 2^-24 log2(N^2) max|map - monopole| is ten times that; adding the monopole and the two passes of
    the smoothing each store the map once more, 4 * 2^-24 max|map|.
    Measured on the MI355X, f32, cuboid box (device deviation from the f64 model / delta_ref / whole bound), unsmoothed:
    N = 16: 4.732e-07 / 2.981e-09 / 2.543e-06, 18: 4.772e-07 / 3.445e-09 / 2.557e-06, 24: 4.755e-07 / 5.158e-09 /
    2.657e-06, 30: 4.817e-07 / 1.289e-08 / 2.849e-06, 72: 5.195e-07 / 3.709e-08 / 4.747e-06; smoothed: 16: 6.397e-07 /
    6.299e-11 / 2.388e-06, 18: 6.389e-07 / 5.338e-11 / 2.387e-06, 24: 6.596e-07 / 1.591e-10 / 2.390e-06, 30: 7.314e-07 /
    2.178e-10 / 2.394e-06, 72: 7.191e-07 / 7.629e-10 / 2.442e-06.  The deviation is the storage of values near 10 (half an
    ulp there is 4.77e-07); the cubic box gives the same figures to 5 per cent."""
    from fastbox_amd import ForegroundModel
    from fastbox_amd import cosmology as ccl
    from fastbox_amd.sky import sky_draw_seed
    box = _box(N, precision, rng="device", box_scale=box_scale)
    geo = {"N": N, "Lx": box.Lx, "Ly": box.Ly}
    r = ccl.comoving_angular_distance(box.cosmo, box.scale_factor)
    ang_x, _ = box.pixel_array()
    fg = ForegroundModel(box)
    for draw, sigma_pix in ((1, None), (2, 3.)):
        got = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10.,
                                        smoothing_scale=None if sigma_pix is None else 3. * (ang_x[1] - ang_x[0]))
        seed = sky_draw_seed(SEED, draw)
        want = sn.foreground_model(geo, r, 57., 1.1, 10., sigma_pix, N, seed, np.float64)
        dev = np.max(np.abs(got - want))
        scale = np.max(np.abs(want - 10.))
        if precision == "f64":
            assert dev < 40 * 1e-12 * max(1., scale), (draw, dev)
        else:
            delta_ref = np.max(np.abs(sn.foreground_model(geo, r, 57., 1.1, 10., sigma_pix, N, seed, np.float32) - want))
            bound = 4 * delta_ref + sn.U32 * (8 * np.log2(N * N) * scale + 4 * np.max(np.abs(want)))
            print("foreground map N=%d %s draw %d: device %.3e delta_ref %.3e bound %.3e" % (
                N, "cuboid" if isinstance(box_scale, tuple) else "cubic", draw, dev, delta_ref, bound))
            assert np.isfinite(delta_ref) and delta_ref > 0
            assert dev <= bound, "draw %d: device deviation %.3e, delta_ref %.3e, bound %.3e" % (draw, dev, delta_ref, bound)


# ---- e. the Gaussian smoothing on its own -----------------------------------------------------------------------------
def _smooth_on_device(box, a, w, r):
    from fastbox_amd import _lib
    from fastbox_amd.sky import _Maps
    m = _Maps(box)
    buf, tmp = m.upload(a), m.empty()
    w = np.ascontiguousarray(w, dtype=np.float64)
    _lib.call("fb_sky_gaussian_filter", box.engine._plan, buf.ptr, tmp.ptr, w.ctypes.data_as(_lib.P_double), int(r),
              box.engine.stream)
    box.engine.sync()
    return m.download(buf)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("N", sn.SIZES)
def test_gaussian_filter_on_constructed_maps(N, precision):
    box = _box(N, precision)
    maps = sn.smoothing_maps(N)
    for r in sn.smoothing_radii(N):
        w = sn.weights_for_radius(r)
        got = {k: _smooth_on_device(box, v, w, r) for k, v in maps.items()}
        for k, v in maps.items():
            held = sn.as_stored(v, precision)
            want = sn.wrap_smooth(held, w, r)
            delta_ref = 1e-12
            if 1 <= r < N:
                delta_ref = max(delta_ref, np.max(np.abs(scipy.ndimage.gaussian_filter(held, sigma=r / 4., mode="wrap") - want)))
            # f32: the map is stored between the passes, off by up to 2^-24 max|in| (positive weights of sum 1), which
            # the second pass averages, and once more at the end: the value of 4 * 2^-24 |value| is the map's largest,
            # not the element's own -- where the smoothed map crosses zero the stored intermediate's rounding remains
            bound = 10 * delta_ref + (4 * sn.U32 * np.max(np.abs(held)) if precision == "f32" else 0.)
            assert np.max(np.abs(got[k] - want)) <= bound, (r, k, np.max(np.abs(got[k] - want)), delta_ref)
            if r == 0:
                assert np.array_equal(got[k], held), (r, k)          # sigma_pix = 0.1: the identity, bit for bit
        # a spike's response: every row and column is a periodic shift of the folded weights
        W = sn.folded_weights(w, r, N)
        assert np.array_equal(got["spikeNN"], np.roll(got["spike00"], (-1, -1), axis=(0, 1))), r
        if 2 * r + 1 <= N:                                           # one term per output element: exact
            first = sn.as_stored(W, precision)                       # the map after the pass along axis 0, column 0
            assert np.array_equal(got["spike00"], sn.as_stored(np.outer(first, W), precision)), r
            assert np.array_equal(W, np.roll(np.concatenate([w, np.zeros(N - 2 * r - 1)]), -r))
        else:
            col = got["spike00"][:, 0]
            assert np.max(np.abs(col - W * W[0])) <= 1e-11 + (4 * sn.U32 * W[0] * W.max() if precision == "f32" else 0.), r


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_gaussian_filter_refuses_a_window_wider_than_its_table(precision):
    from fastbox_amd import _lib
    from fastbox_amd.sky import _Maps
    N = 18
    box = _box(N, precision)
    m = _Maps(box)
    a = np.random.RandomState(3).normal(size=(N, N))
    buf, tmp = m.upload(a), m.empty()
    r = 4096                                                         # 2 r + 1 = 8193 > the 8192 doubles of the table
    w = np.full(2 * r + 1, 1. / (2 * r + 1))
    with pytest.raises(_lib.FastBoxError) as e:
        _lib.call("fb_sky_gaussian_filter", box.engine._plan, buf.ptr, tmp.ptr, w.ctypes.data_as(_lib.P_double), r,
                  box.engine.stream)
    assert e.value.code == -1                                        # FB_ERR_INVALID
    box.engine.sync()
    assert np.array_equal(m.download(buf), sn.as_stored(a, precision))
    r = 4095                                                         # the widest window it takes: a flat one is the mean
    w = np.full(2 * r + 1, 1. / (2 * r + 1))
    got = _smooth_on_device(box, a, w, r)
    want = sn.wrap_smooth(sn.as_stored(a, precision), w, r)
    assert np.max(np.abs(got - want)) <= 1e-11 + (4 * sn.U32 * np.max(np.abs(want)) if precision == "f32" else 0.)


# ---- f. foreground cube ------------------------------------------------------------------------------------------------
def _check_cube(box, amps, idx, precision):
    from fastbox_amd import ForegroundModel
    N = box.N
    freqs = box.freq_array()
    got = np.asarray(ForegroundModel(box).construct_cube(amps, idx, freq_ref=130.))
    a = sn.as_stored(amps, precision)
    al = idx if isinstance(idx, float) else sn.as_stored(idx, precision)
    want = so.construct_cube(a, al, freqs, freq_ref=130.)
    assert got.shape == (N, N, N)
    zero = want == 0
    assert np.array_equal(got[zero], want[zero]) and np.array_equal(np.signbit(got[~zero]), np.signbit(want[~zero]))
    rel = sn.relative_per_channel(got, want)
    if precision == "f64":
        assert np.all(rel < 1e-12), (np.argmax(rel), rel.max())
        return None
    rel_ref = sn.relative_per_channel(sn.fg_cube_f32(amps, idx, freqs / 130.), want)
    bound = 4 * rel_ref + 2 * sn.U32
    worst = np.argmax(rel / bound)
    assert np.all(rel <= bound), "channel %d: device %.3e, delta_ref %.3e (relative); over all channels %.3e, %.3e" % (
        worst, rel[worst], rel_ref[worst], rel.max(), rel_ref.max())
    return rel.max(), rel_ref.max()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("N", sn.SIZES)
def test_foreground_cube_map_and_scalar_index(N, precision):
    """amps[x, y] ratio[z] ** alpha[x, y] channel by channel, relative: zeros and signs carry through.  f32: within
    4 delta_ref + 2 * 2^-24 of the f64 statement, delta_ref the numpy float32 restatement of the kernel's expression.
    Measured on the MI355X, f32 (largest relative device deviation / largest delta_ref over the channels), index map:
    N = 16: 6.504e-07 / 6.504e-07, 18: 6.174e-07 / 6.174e-07, 24: 6.252e-07 / 6.325e-07, 30: 6.501e-07 / 6.593e-07,
    72: 6.770e-07 / 7.031e-07; scalar -2.7: 4.368e-07, 5.124e-07, 3.969e-07, 3.915e-07, 5.089e-07, each equal to its
    delta_ref; scalar 3.5: 5.821e-07 / 5.821e-07, 4.879e-07 / 4.915e-07, 5.883e-07 / 6.474e-07, 5.416e-07 / 5.416e-07,
    6.674e-07 / 7.051e-07; N = 270, scalar -2.7: 5.156e-07 / 5.156e-07."""
    box = _box(N, precision)
    amps, alpha = sn.cube_inputs(N)
    for idx in (alpha, -2.7, 3.5):
        res = _check_cube(box, amps, idx, precision)
        if res:
            print("foreground cube N=%d %s: device %.3e delta_ref %.3e" % ((N, "map" if idx is alpha else idx) + res))


def test_foreground_cube_second_partial_trip_of_a_256_thread_block():
    """N = 270, the smallest size above 256: the block is 256 threads and its second trip covers 14 channels."""
    N = 270
    box = _box(N, "f32")
    amps, _ = sn.cube_inputs(N)
    res = _check_cube(box, amps, -2.7, "f32")
    print("foreground cube N=270 scalar: device %.3e delta_ref %.3e" % res)


# ---- g. the chain at N = 18 ---------------------------------------------------------------------------------------------
def test_chain_at_n18_foregrounds_noise_beam_and_bandpass():
    """Foreground cube + noise cube, beam convolution (transform size 2 N = 36) and the angular band-pass at N = 18,
    N % 4 = 2, f64, host draws: each step against its oracle at the tolerances of tests/test_generic_grid_gpu.py."""
    from fastbox_amd import BeamModel, ForegroundModel, NoiseModel, _lib, filters
    from fastbox_amd import cosmology as ccl
    from fastbox_amd.device import FULL
    from oracle import beam_oracle as beo
    from oracle import pca_oracle as po
    N, tol = 18, 1e-12
    box = _box(N, "f64", box_scale=sn.CUBOID)
    geo = {"N": N, "Lx": box.Lx, "Ly": box.Ly}
    r = ccl.comoving_angular_distance(box.cosmo, box.scale_factor)
    ang_x, ang_y = box.pixel_array()
    pix = ang_x[1] - ang_x[0]
    freqs = box.freq_array()
    sigma = _sigma(box)
    fg, nm = ForegroundModel(box), NoiseModel(box)
    np.random.seed(12)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., smoothing_scale=2. * pix)
    alpha = fg.realise_spectral_index(mean_spec_idx=-2.7, std_spec_idx=0.1, smoothing_scale=1.5 * pix)
    fg_cube = fg.construct_cube(fg_map, alpha, freq_ref=130.)
    noise = nm.realise_radiometer_noise(**sn.RADIOMETER)
    np.random.seed(12)
    omap = so.foreground_amp(geo, r, 57., 1.1, 10., sigma_pix=2.)
    oalpha = so.spectral_index(N, -2.7, 0.1, 1.5)
    onoise = so.radiometer_noise((N, N, N), sigma)
    assert np.max(np.abs(fg_map - omap)) < 40 * tol * max(1., np.max(np.abs(omap - 10.)))
    assert np.max(np.abs(alpha - oalpha)) < 3 * tol * np.max(np.abs(oalpha))
    ocube = so.construct_cube(fg_map, alpha, freqs, freq_ref=130.)
    assert np.max(np.abs(np.asarray(fg_cube) / ocube - 1)) < tol
    assert np.max(np.abs(np.asarray(noise) / onoise - 1)) < tol
    data = fg_cube + noise
    host = np.asarray(data)
    assert np.max(np.abs(host - (ocube + onoise))) < tol * np.max(np.abs(ocube + onoise))

    beam_cube = beo.test_beam_cube(ang_x, ang_y, freqs, fwhm_deg=0.2 * (ang_x[-1] - ang_x[0]))

    class FixtureBeam(BeamModel):
        def beam_cube(self, pol=None):
            return beam_cube

    beam = FixtureBeam(box)
    want = beo.convolve_fft(beam_cube, host)
    assert np.max(np.abs(np.asarray(beam.convolve_fft(data)) - want)) < tol * np.max(np.abs(want))
    want = beo.convolve_real(beam_cube, host)
    assert np.max(np.abs(want - beo.convolve_real_direct(beam_cube, host))) < tol * np.max(np.abs(want))
    assert np.max(np.abs(np.asarray(beam.convolve_real(data)) - want)) < tol * np.max(np.abs(want))

    scale = np.max(np.abs(host))
    got = np.asarray(filters.angular_bandpass_filter(data, 0.05, 0.3, d=1.))
    assert np.max(np.abs(got - po.angular_bandpass_filter(host, 0.05, 0.3, d=1.))) < tol * scale
    # kmin = 0, kmax = inf keeps every mode: k_mask_xy returns early on mask == 1, so the result is the transform there
    # and back of the cube bit for bit (the two transforms themselves round), and the cube to the tolerance
    eng = box.engine
    trip = eng.empty(FULL)
    _lib.call("fb_real_to_complex", eng._plan, data.ptr, trip.ptr, eng.stream)
    _lib.call("fb_fft_transverse", eng._plan, trip.ptr, -1, eng.stream)
    _lib.call("fb_fft_transverse", eng._plan, trip.ptr, +1, eng.stream)
    trip.invalidate()
    everything = np.asarray(filters.angular_bandpass_filter(data, 0., np.inf, d=1.))
    assert np.array_equal(everything, np.asarray(trip))
    assert np.max(np.abs(everything - host)) < tol * scale
    nothing = np.asarray(filters.angular_bandpass_filter(data, 10., 11., d=1.))
    assert nothing.shape == (N, N, N) and np.array_equal(nothing, np.zeros((N, N, N), dtype=complex))
