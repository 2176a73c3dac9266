"""GPU: Minkowski functionals of excursion sets (fb_minkowski.hip; fastbox_amd.minkowski, CosmoBox.minkowski_functionals) in both
precisions.  Every count is compared with assert_array_equal on int64: with the literal integers of the constructed cases of
tests/minkowski_cases.py, and with the numpy statement of tests/minkowski_numpy.py -- which tests/test_minkowski_cases_cpu.py
validates on its own -- applied to the field as the plan stores it.  Nothing is larger than 64^3."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, DeviceArray, _lib, default_cosmo, minkowski as mk
from tests import minkowski_cases as mc
from tests import minkowski_numpy as mn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
CUBOID = (32., 48., 80.)
NTS_3D = (1, 2, 25, 100, 256)          # 16, 16, 16, 8 and 4 interleaved copies of the workgroup histogram
NTS_2D = (1, 25, 40, 100, 256)         # 64, 64, 32, 16 and 8 channels per tile


@functools.lru_cache(maxsize=None)
def _box(prec, N, L=None):
    return CosmoBox(cosmo=default_cosmo, box_scale=(2. * N if L is None else L), nsamp=N, realise_now=False, precision=prec,
                    rng="device", seed=5)


def _thresholds(nt, seed=0):
    """non-uniform, strictly ascending, inside and a little beyond unit-normal data"""
    t = np.unique(np.random.RandomState(100 + nt + seed).normal(scale=1.2, size=nt))
    assert t.size == nt
    return t


def _check_3d(mf, want):
    for key in ("n3", "n2", "n1", "n0"):
        assert mf.__dict__[key].dtype == np.int64
        np.testing.assert_array_equal(mf.__dict__[key], want[key], err_msg=key)
    assert mf.n_nan == want["n_nan"]
    np.testing.assert_array_equal(mf.euler, mn.euler_3d(want))
    np.testing.assert_array_equal(mf.genus, -0.5 * mn.euler_3d(want))


def _check_2d(mf, want):
    for key in ("n2", "n1", "n0", "n_nan"):
        assert mf.__dict__[key].dtype == np.int64
        np.testing.assert_array_equal(mf.__dict__[key], want[key], err_msg=key)
    np.testing.assert_array_equal(mf.euler, mn.euler_2d(want))


# ---- constructed cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", (16, 18, 30))
def test_constructed_bodies(N, prec):
    """Every body on every axis order: the literal counts (16 is the tile's multiple; 18 and 30 are N % 4 = 2 and no power of
    two, so tiles and waves do not divide the grid)."""
    box = _box(prec, N)
    for name, field, e in mc.cases_3d(N):
        mf = mk.minkowski_functionals(field, thresholds=[mc.THRESHOLD], box=box)
        got = (int(mf.n3[0]), tuple(int(v) for v in mf.n2[:, 0]), tuple(int(v) for v in mf.n1[:, 0]), int(mf.n0[0]), int(mf.euler[0]))
        assert got == (e["n3"], e["n2"], e["n1"], e["n0"], e["chi"]), name
        assert mf.n_nan == 0 and mf.v0[0] == e["n3"] / float(N) ** 3


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", (16, 18, 30))
def test_constructed_shapes_per_channel(N, prec):
    """Adjacent channels of one cube hold different shapes: a channel / pixel-axis transposition would show."""
    box = _box(prec, N)
    cube, e = mc.channel_cube(N)
    mf = mk.minkowski_functionals(cube, thresholds=[mc.THRESHOLD], per_channel=True, box=box)
    np.testing.assert_array_equal(mf.n2[:, 0], e["n2"])
    np.testing.assert_array_equal(mf.n1[:, :, 0], e["n1"])
    np.testing.assert_array_equal(mf.n0[:, 0], e["n0"])
    np.testing.assert_array_equal(mf.euler[:, 0], e["chi"])
    np.testing.assert_array_equal(mf.n_nan, np.zeros(N, dtype=np.int64))
    assert mf.v0.shape == mf.v1.shape == mf.v2.shape == (N, 1)


@pytest.mark.parametrize("prec", PRECS)
def test_cuboid_box_uses_the_areas_per_orientation(prec):
    N = 16
    box = _box(prec, N, CUBOID)
    rod = [f for n, f, _ in mc.cases_3d(N) if n == "rod along x, axes xyz"][0]
    mf = mk.minkowski_functionals(rod, thresholds=[mc.THRESHOLD], box=box)
    a, b, c = [s / N for s in CUBOID]
    V = CUBOID[0] * CUBOID[1] * CUBOID[2]
    assert mf.L == CUBOID
    # a rod of cross-section b x c around the periodic x axis: surface 2 (b + c) Lx, no end faces; mean breadth from its 4 edges
    assert mf.v1[0] == pytest.approx(2. * (N * a * c + N * a * b) / (9. * V), rel=1e-14)
    assert mf.v2[0] == pytest.approx(2. * (N * a) / (9. * V), rel=1e-14) and mf.v3[0] == 0.
    field = np.random.RandomState(2).normal(size=(N, N, N))
    t = _thresholds(25)
    mf = mk.minkowski_functionals(field, thresholds=t, box=box)
    want = mn.counts_3d(mn.stored(field, DT[prec]), t)
    _check_3d(mf, want)
    for got, ref in zip((mf.v0, mf.v1, mf.v2, mf.v3), mk.minkowski_from_counts(want["n3"], want["n2"], want["n1"], want["n0"], N, CUBOID)):
        np.testing.assert_array_equal(got, ref)
    cubic = mk.minkowski_from_counts(want["n3"], want["n2"], want["n1"], want["n0"], N, V ** (1. / 3.))
    assert np.max(np.abs(mf.v1 - cubic[1])) > 1e-3 * np.max(np.abs(mf.v1))
    # per channel: the perimeter takes a_x and a_y
    mfc = mk.minkowski_functionals(field, thresholds=t, per_channel=True, box=box)
    wantc = mn.counts_per_channel(mn.stored(field, DT[prec]), t)
    _check_2d(mfc, wantc)
    for got, ref in zip((mfc.v0, mfc.v1, mfc.v2), mk.minkowski_from_counts_2d(wantc["n2"], wantc["n1"], wantc["n0"], N, CUBOID[:2])):
        np.testing.assert_array_equal(got, ref)


# ---- random fields ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_field(N):
    f = np.random.RandomState(N).normal(size=(N, N, N))
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nt", NTS_3D)
@pytest.mark.parametrize("N", (16, 18, 32, 64))
def test_random_field_is_the_statement(N, nt, prec):
    box, t = _box(prec, N), _thresholds(nt)
    mf = mk.minkowski_functionals(_random_field(N), thresholds=t, box=box)
    _check_3d(mf, mn.counts_3d(mn.stored(_random_field(N), DT[prec]), t))
    assert mf.nu is None and mf.thresholds.shape == (nt,) and mf.n2.shape == mf.n1.shape == (3, nt)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nt", NTS_2D)
@pytest.mark.parametrize("N", (16, 18, 32))
def test_random_cube_per_channel_is_the_statement(N, nt, prec):
    box, t = _box(prec, N), _thresholds(nt)
    mf = mk.minkowski_functionals(_random_field(N), thresholds=t, per_channel=True, box=box)
    _check_2d(mf, mn.counts_per_channel(mn.stored(_random_field(N), DT[prec]), t))
    assert mf.n2.shape == mf.n0.shape == (N, nt) and mf.n1.shape == (2, N, nt) and mf.n_nan.shape == (N,)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nt", NTS_2D)
def test_threshold_table_with_a_row_per_channel(nt, prec):
    N = 18
    box = _box(prec, N)
    t = np.array([_thresholds(nt, seed=1000 * (c + 1)) + 0.05 * c for c in range(N)])
    field = np.array(_random_field(N))
    field[3, 4, 5] = field[N - 1, N - 1, 5] = field[0, 0, N - 1] = np.nan
    mf = mk.minkowski_functionals(field, thresholds=t, per_channel=True, box=box)
    want = mn.counts_per_channel(mn.stored(field, DT[prec]), t)
    _check_2d(mf, want)
    assert mf.n_nan[5] == 2 and mf.n_nan[N - 1] == 1 and mf.n_nan.sum() == 3 and mf.thresholds.shape == (N, nt)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", (16, 18))
def test_thresholds_outside_the_data_ties_and_constant_fields(N, prec):
    box, n = _box(prec, N), N ** 3
    f = _random_field(N)
    lo, hi = float(f.min()), float(f.max())
    below = mk.minkowski_functionals(f, thresholds=[lo - 3., lo - 2., lo - 1.], box=box)
    above = mk.minkowski_functionals(f, thresholds=[hi + 1., hi + 2., hi + 3.], box=box)
    for key in ("n3", "n0"):
        np.testing.assert_array_equal(below.__dict__[key], [n] * 3)
        np.testing.assert_array_equal(above.__dict__[key], [0] * 3)
    np.testing.assert_array_equal(below.n2, np.full((3, 3), n))
    np.testing.assert_array_equal(below.euler, [0] * 3)
    # integers with the thresholds on them: >= and not >
    ints = np.random.RandomState(7).randint(-3, 4, size=(N, N, N)).astype(np.float64)
    t = np.arange(-3., 4.)
    mf = mk.minkowski_functionals(ints, thresholds=t, box=box)
    _check_3d(mf, mn.counts_3d(ints, t))
    np.testing.assert_array_equal(mf.n3, [np.sum(ints >= v) for v in t])
    assert mf.n3[0] == n and mf.n3[-1] == np.sum(ints == 3.) > 0
    _check_2d(mk.minkowski_functionals(ints, thresholds=t, per_channel=True, box=box), mn.counts_per_channel(ints, t))
    # a field equal everywhere to a threshold
    flat = mk.minkowski_functionals(np.full((N, N, N), 0.75), thresholds=[0.5, 0.75, 1.], box=box)
    np.testing.assert_array_equal(flat.n3, [n, n, 0])
    np.testing.assert_array_equal(flat.n1, [[n, n, 0]] * 3)
    np.testing.assert_array_equal(flat.n0, [n, n, 0])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", (16, 18, 32))
def test_nan_and_infinite_voxels(N, prec):
    """On the seam (index 0 and N - 1 of each axis, the corner) and in the interior; n_nan exact."""
    box, M = _box(prec, N), N - 1
    f = np.array(_random_field(N))
    nans = [(0, 0, 0), (M, M, M), (M, 0, 5), (3, M, 0), (7, 8, 9), (7, 8, 10)]
    pinf = [(0, M, M), (M, 3, 4), (6, 6, 6)]
    ninf = [(M, M, 0), (0, 5, M), (9, 9, 9)]
    for v in nans:
        f[v] = np.nan
    for v in pinf:
        f[v] = np.inf
    for v in ninf:
        f[v] = -np.inf
    t = np.concatenate([[-1e300], _thresholds(25), [1e300]])
    mf = mk.minkowski_functionals(f, thresholds=t, box=box)
    want = mn.counts_3d(mn.stored(f, DT[prec]), t)
    _check_3d(mf, want)
    assert mf.n_nan == len(nans) and mf.n3[-1] == len(pinf) and mf.n3[0] == N ** 3 - len(nans) - len(ninf)
    mfc = mk.minkowski_functionals(f, thresholds=t, per_channel=True, box=box)
    _check_2d(mfc, mn.counts_per_channel(mn.stored(f, DT[prec]), t))
    assert mfc.n_nan.sum() == len(nans) and mfc.n_nan[0] == 2


# ---- nu ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_nu_thresholds_follow_the_moments(prec):
    """f64 plan: the mean, sigma and thresholds are those of the host's fp64 moments to 1e-12 relative, each against its own value
    (no threshold of this field is near 0).  Both plans: the counts are the statement's at the thresholds the call reports."""
    N = 32
    box = _box(prec, N)
    f = 0.3 + 1.7 * _random_field(N) * (1. + 0.5 * np.arange(N)[None, None, :] / N)       # sigma varies along the channels
    s = mn.stored(f, DT[prec])
    nu = np.linspace(-2.5, 2.5, 11)
    mf = mk.minkowski_functionals(f, nu=nu, box=box)
    _check_3d(mf, mn.counts_3d(s, mf.thresholds))
    np.testing.assert_array_equal(mf.nu, nu)
    mfc = mk.minkowski_functionals(f, nu=nu, per_channel=True, box=box)
    _check_2d(mfc, mn.counts_per_channel(s, mfc.thresholds))
    assert mfc.thresholds.shape == (N, 11) and mfc.mean.shape == mfc.sigma.shape == (N,)
    m, sd = s.mean(), s.std()
    mc_, sdc = s.mean(axis=(0, 1)), s.std(axis=(0, 1))
    tol = 1e-12 if prec == "f64" else 1e-6            # f32 plan: the bound of a reduction carried in the plan's own precision
    np.testing.assert_allclose([mf.mean, mf.sigma], [m, sd], rtol=tol, atol=0.)
    np.testing.assert_allclose(mfc.mean, mc_, rtol=tol, atol=0.)
    np.testing.assert_allclose(mfc.sigma, sdc, rtol=tol, atol=0.)
    np.testing.assert_allclose(mf.thresholds, m + nu * sd, rtol=tol, atol=0.)
    np.testing.assert_allclose(mfc.thresholds, mc_[:, None] + nu[None, :] * sdc[:, None], rtol=tol, atol=0.)
    # with thresholds= the moments are formed when first read, and are the same numbers
    lazy = mk.minkowski_functionals(f, thresholds=mf.thresholds, box=box)
    assert callable(lazy._moments) and lazy.mean == mf.mean and lazy.sigma == mf.sigma and not callable(lazy._moments)
    # the default: nu = linspace(-3, 3, 25)
    d = mk.minkowski_functionals(f, box=box)
    np.testing.assert_array_equal(d.nu, np.linspace(-3., 3., 25))
    # a channel without variance
    g = np.array(f)
    g[:, :, 7] = 2.
    with pytest.raises(ValueError, match="sigma = 0"):
        mk.minkowski_functionals(g, nu=nu, per_channel=True, box=box)


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    N = 16
    box, other = _box("f32", N), _box("f64", N)
    f = np.array(_random_field(N))
    dev = box.engine.upload(f, "real")
    for bad in ([1., 0.5], [0., 0.], [0., 1., 1.], [], np.linspace(0., 1., 257), [0., np.nan], [0., np.inf], np.zeros((2, 3))):
        with pytest.raises(ValueError):
            mk.minkowski_functionals(dev, thresholds=bad)
    with pytest.raises(ValueError):
        mk.minkowski_functionals(dev, thresholds=np.zeros((N, 3)), per_channel=True)            # rows not ascending
    with pytest.raises(ValueError):
        mk.minkowski_functionals(dev, thresholds=np.tile(np.arange(3.), (N, 1)))                # a table without per_channel
    with pytest.raises(ValueError):
        mk.minkowski_functionals(dev, thresholds=[0.], nu=[0.])
    with pytest.raises(ValueError):
        mk.minkowski_functionals(dev, nu=[1., 0.])
    with pytest.raises(TypeError):
        mk.minkowski_functionals(f + 1j * f, thresholds=[0.], box=box)
    with pytest.raises(TypeError):
        mk.minkowski_functionals(box.engine.fft_r2c(dev), thresholds=[0.])
    with pytest.raises(TypeError):
        mk.minkowski_functionals(f, thresholds=[0.])                                             # a host array without box=
    with pytest.raises(ValueError):
        mk.minkowski_functionals(f[:, :, :8], thresholds=[0.], box=box)
    with pytest.raises(ValueError):
        mk.minkowski_functionals(dev, thresholds=[0.], box=other)                                # a field of another box
    with pytest.raises(ValueError):
        other.minkowski_functionals(dev, thresholds=[0.])
    # the C ABI refuses the same with FB_ERR_INVALID
    eng = box.engine
    out, nan = (ctypes.c_uint64 * (8 * 300))(), (ctypes.c_uint64 * N)()

    def call(t, nt, mode):
        t = np.ascontiguousarray(t, dtype=np.float64)
        _lib.call("fb_minkowski_counts", eng._plan, dev.ptr, t.ctypes.data_as(_lib.P_double), nt, mode, out, nan, eng.stream)
    for t, nt, mode in (([1., 0.5], 2, 0), ([0., 0.], 2, 0), ([0.], 0, 0), (np.arange(257.), 257, 0), ([0., np.inf], 2, 0),
                        ([0.], 1, 3), ([0.], 1, -1), (np.zeros((N, 2)), 2, 2)):
        with pytest.raises(_lib.FastBoxError) as err:
            call(t, nt, mode)
        assert err.value.code == -1
    call([0.], 1, 0)                                                                             # and takes a good call after them
    assert out[0] == np.sum(mn.stored(f, np.float32) >= 0.)


# ---- repeatability, device-made fields, the box method, spectral moments -----------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_give_identical_arrays(prec):
    N = 32
    box = _box(prec, N)
    f = box.engine.upload(0.5 + _random_field(N), "real")
    for kw in (dict(), dict(per_channel=True)):
        a, b = mk.minkowski_functionals(f, **kw), mk.minkowski_functionals(f, **kw)
        for key in ("thresholds", "mean", "sigma", "n2", "n1", "n0", "euler", "n_nan", "v0", "v1", "v2"):
            np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)


@pytest.mark.parametrize("prec", PRECS)
def test_slices_of_the_box_tie_the_two_kernels(prec):
    """A z-slice's pixels, x-edges, y-edges and vertices are the box's cells, y-faces, x-faces and z-edges in that slice."""
    N, t = 30, _thresholds(25)
    f = _box(prec, N).engine.upload(_random_field(N), "real")
    a, c = mk.minkowski_functionals(f, thresholds=t), mk.minkowski_functionals(f, thresholds=t, per_channel=True)
    np.testing.assert_array_equal(c.n2.sum(axis=0), a.n3)
    np.testing.assert_array_equal(c.n1[0].sum(axis=0), a.n2[1])
    np.testing.assert_array_equal(c.n1[1].sum(axis=0), a.n2[0])
    np.testing.assert_array_equal(c.n0.sum(axis=0), a.n1[2])


@pytest.mark.parametrize("prec", PRECS)
def test_device_generated_field_and_the_box_method(prec):
    """A Gaussian realisation made on the device at 64^3: the counts of the statement applied to its download; the box method
    takes box.delta_x by default and leaves the box's state alone."""
    N = 64
    box = CosmoBox(cosmo=default_cosmo, box_scale=4. * N, nsamp=N, realise_now=False, precision=prec, rng="device", seed=11)
    box.realise_density()
    host = np.asarray(box.delta_x)
    mf = box.minkowski_functionals()
    assert isinstance(box.delta_x, DeviceArray) and mf.n3.shape == (25,) and not mf.per_channel
    _check_3d(mf, mn.counts_3d(host, mf.thresholds))
    assert mf.n3[0] > 0.99 * N ** 3 and mf.n3[-1] < 0.01 * N ** 3 and np.all(np.diff(mf.n3) <= 0)
    mfc = box.minkowski_functionals(per_channel=True, nu=[-1., 0., 1.])
    _check_2d(mfc, mn.counts_per_channel(host, mfc.thresholds))
    np.testing.assert_array_equal(np.asarray(box.delta_x), host)
    # a Gaussian field: the measured functionals follow the expectations of its own spectral moments
    s0, s1 = mk.spectral_moments(box, box.delta_x)
    assert s0 == pytest.approx(mf.sigma, rel=1e-4)
    theory = mk.gaussian_minkowski(mf.nu, s0, s1)
    assert np.max(np.abs(mf.v0 - theory[0])) < 0.02


def test_spectral_moments_of_a_plane_wave():
    """sigma0 = amplitude / sqrt(2) and sigma1 / sigma0 = |k| for one plane wave: exactly on a cubic box (every mode of a k^2 bin
    has the same |k| at N = 16), and within the bin width on a cuboid one -- k^2 is off by at most k_corner^2 / 1024."""
    N, m = 16, (2, 1, 3)
    x = np.arange(N)
    phase = 2. * np.pi * (m[0] * x[:, None, None] + m[1] * x[None, :, None] + m[2] * x[None, None, :]) / N
    for L, exact in (((32., 32., 32.), True), (CUBOID, False)):
        box = _box("f64", N, L[0] if exact else L)
        k2 = (2. * np.pi) ** 2 * sum((mi / Li) ** 2 for mi, Li in zip(m, L))
        s0, s1 = mk.spectral_moments(box, 3. * np.cos(phase + 0.4) + 5.)
        assert s0 == pytest.approx(3. / np.sqrt(2.), rel=1e-10)
        width = (np.pi * N) ** 2 * sum(1. / Li ** 2 for Li in L) / 1024.
        assert abs((s1 / s0) ** 2 - k2) <= (1e-10 * k2 if exact else width)
