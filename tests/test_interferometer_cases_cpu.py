"""CPU: the numpy statement of the interferometer (tests/interferometer_numpy.py), the constructed cases
(tests/interferometer_cases.py) and the host helpers of fastbox_amd/interferometer.py, validated on their own."""
import numpy as np
import pytest

from fastbox_amd import interferometer as itf
from tests import interferometer_cases as ic
from tests import interferometer_numpy as inp

GEOMS = ("n16", "n18", "cuboid")


def _mirror(S):
    """S[-m mod N] over both transverse axes."""
    N = S.shape[0]
    idx = (-np.arange(N)) % N
    return S[idx][:, idx]


@pytest.mark.parametrize("geom", GEOMS + ("n30",))
def test_counts_are_symmetric_and_sum_to_twice_the_accepted(geom):
    N, sx, sy = ic.tables(geom)
    assert sx.dtype == sy.dtype == np.float64 and sx.shape == sy.shape == (N,) and np.all(sx > 0) and np.all(sy > 0)
    for name, samples, mult in ic.cases(N, sx, sy):
        S = inp.coverage(N, samples, mult, sx, sy)
        tot, ncell = inp.channel_sums(S)
        assert S.dtype == np.int32 and S.min() >= 0, name
        assert np.array_equal(S, _mirror(S)), name
        assert np.array_equal(tot, 2 * inp.accepted_multiplicity(N, samples, mult, sx, sy)), name
        assert np.all(ncell <= N * N) and np.array_equal(ncell > 0, tot > 0), name


def test_channel_tables_follow_the_definition():
    N, scale = ic.GEOMETRIES["cuboid"]
    hb = ic.HostBox(N, scale)
    sx, sy = itf.channel_scales(hb)
    du, dv = itf.uv_cell(hb)
    r = itf._ccl.comoving_angular_distance(hb.cosmo, 1. / (1. + hb.redshift))
    assert du == r / hb.Lx and dv == r / hb.Ly and du != dv
    nu = hb.freq_array()
    assert np.array_equal(sx, nu * 1e6 / 299792458 / du) and np.array_equal(sy, nu * 1e6 / 299792458 / dv)
    # du is one over the field of view N dtheta_x with dtheta_x = (Lx / N) / r
    assert np.isclose(du, 1. / (N * (hb.Lx / N) / r), rtol=1e-15)


@pytest.mark.parametrize("geom", GEOMS)
def test_special_cases(geom):
    N, sx, sy = ic.tables(geom)
    byname = {name: (s, m) for name, s, m in ic.cases(N, sx, sy)}
    # expanded copies and one sample with their multiplicity: identical counts
    a = inp.coverage(N, *byname["copies-expanded"], sx, sy)
    b = inp.coverage(N, *byname["copies-collapsed"], sx, sy)
    assert np.array_equal(a, b) and a.max() == ic.N_COPIES
    # the zero baseline is its own conjugate: 2 m in cell (0, 0) of every channel
    z = inp.coverage(N, *byname["zero-baseline"], sx, sy)
    assert np.all(z[0, 0, :] == 6) and z.sum() == 6 * N
    # no samples: nothing
    assert not inp.coverage(N, *byname["random0"], sx, sy).any()
    # every cell of every channel
    assert inp.coverage(N, *byname["everywhere"], sx, sy).min() >= 1
    # part of the band is empty, part is not
    tot = inp.channel_sums(inp.coverage(N, *byname["band-edge"], sx, sy))[0]
    assert (tot == 0).any() and (tot > 0).any()
    # the random sets lose samples in every channel, and keep at least a quarter
    acc = inp.accepted_multiplicity(N, *byname["random1000"], sx, sy)
    assert np.all(acc < 1000) and np.all(acc > 250) and acc[-1] > acc[0]


@pytest.mark.parametrize("N", (16, 18))
def test_edge_set_pins_ties_and_the_grid_edge(N):
    sx, sy = ic.edge_tables(N)
    samples = ic.edge_set(N)
    S = inp.coverage(N, samples, None, sx, sy)
    # the same rule sample by sample with Python's round() (round-half-to-even on exact halves), channel 0
    want = np.zeros((N, N), dtype=np.int64)
    for bx, by in samples:
        a, b = round(bx * 0.5), round(by * 0.5)
        if abs(a) <= N // 2 and abs(b) <= N // 2:
            want[a % N, b % N] += 1
            want[-a % N, -b % N] += 1
    for c in range(N):
        assert np.array_equal(S[:, :, c], want)
    one = lambda bx, by: inp.coverage(N, [[bx, by]], None, sx, sy)[:, :, 0]
    assert one(1., 0.)[0, 0] == 2 and one(3., 0.)[2, 0] == 1 and one(5., 0.)[2, 0] == 1          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert one(-3., 0.)[N - 2, 0] == 1 and one(-3., 0.)[2, 0] == 1
    assert one(float(N), 0.)[N // 2, 0] == 2 and one(-float(N), 0.)[N // 2, 0] == 2              # +-N/2 fold onto row N/2
    assert one(N + 2., 0.).sum() == 0 and one(0., -(N + 2.)).sum() == 0                          # the next one out
    assert one(N + 1., 0.).sum() == (2 if (N // 2) % 2 == 0 else 0)                              # N/2 + 1/2 goes to even


def test_upper_channels_empty():
    N = 16
    sx, sy = ic.upper_empty_tables(N)
    tot, ncell = inp.channel_sums(inp.coverage(N, ic.upper_empty_set(N), None, sx, sy))
    assert np.all(tot[:N // 2] == 100) and np.all(tot[N // 2:] == 0) and np.all(ncell[N // 2:] == 0)


# ---- host helpers ------------------------------------------------------------------------------------------------------------
def test_rotation_synthesis():
    rs = np.random.RandomState(0)
    bl = rs.normal(0., 30., (20, 3))
    lat = np.radians(-30.7)
    uv = itf.rotation_synthesis(bl, lat, lat, [0.])
    assert uv.shape == (20, 2) and np.allclose(uv, bl[:, :2], rtol=0, atol=1e-12)       # H = 0, dec = latitude: (u, v) = (E, N)
    H = np.linspace(-1., 1., 7)
    uv = itf.rotation_synthesis(bl, lat, np.pi / 2, H).reshape(20, 7, 2)                # baseline-major
    X = -bl[:, 1] * np.sin(lat) + bl[:, 2] * np.cos(lat)
    assert np.allclose(np.hypot(uv[..., 0], uv[..., 1]), np.hypot(X, bl[:, 0])[:, None], rtol=1e-13)
    flat = bl.copy()
    flat[:, 2] = 0.
    uv = itf.rotation_synthesis(flat[:, :2], np.pi / 2, np.pi / 2, H).reshape(20, 7, 2)   # at the pole: lengths preserved
    assert np.allclose(np.hypot(uv[..., 0], uv[..., 1]), np.hypot(flat[:, 0], flat[:, 1])[:, None], rtol=1e-13)
    assert np.array_equal(itf.rotation_synthesis(flat[:, :2], lat, 0.3, H), itf.rotation_synthesis(flat, lat, 0.3, H))


def test_array_layouts_and_baselines():
    for n in (1, 2, 3, 11):
        xy = itf.hex_array(n, 14.6)
        assert xy.shape == (3 * n * n - 3 * n + 1, 2) and np.allclose(xy.mean(axis=0), 0., atol=1e-9)
        if n > 1:
            d = np.hypot(*(xy[:, None, :] - xy[None, :, :]).transpose(2, 0, 1))
            assert np.isclose(np.min(d[d > 0]), 14.6)
    assert itf.hex_array(11, 14.6).shape[0] == 331
    g = itf.grid_array(4, 3, 10.)
    assert g.shape == (12, 2) and len({tuple(p) for p in g}) == 12
    bl = itf.baselines_from_antennas(g)
    assert bl.shape == (12 * 11 // 2, 2)
    assert np.array_equal(bl[0], g[1] - g[0])
    assert itf.baselines_from_antennas(np.zeros((5, 3))).shape == (10, 3)
    with pytest.raises(ValueError):
        itf.baselines_from_antennas(np.zeros((5, 4)))


def test_collapse_samples_round_trip():
    bl = itf.baselines_from_antennas(itf.grid_array(5, 5, 7.))          # a redundant array
    uniq, mult = itf.collapse_samples(bl)
    assert mult.dtype == np.int32 and mult.sum() == bl.shape[0] and uniq.shape[0] < bl.shape[0] and mult.min() >= 1
    back = np.repeat(uniq, mult, axis=0)
    key = lambda s: s[np.lexsort((s[:, 1], s[:, 0]))]
    assert np.array_equal(key(back), key(bl))
    N, sx, sy = ic.tables("n16")
    scale = ic.reach(N, sx) / 40.
    assert np.array_equal(inp.coverage(N, bl * scale, None, sx, sy), inp.coverage(N, uniq * scale, mult, sx, sy))
    u0, m0 = itf.collapse_samples(np.zeros((0, 2)))
    assert u0.shape == (0, 2) and m0.shape == (0,)


# ---- the operators -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("weighting", ("natural", "uniform"))
def test_dirty_cube_is_real_psf_is_one_empty_channels_are_zero(geom, weighting):
    N, sx, sy = ic.tables(geom)
    byname = {name: (s, m) for name, s, m in ic.cases(N, sx, sy)}
    cube = ic.smooth_cube(N)
    for name in ("random1000", "random65-mult", "band-edge", "random0"):
        S = inp.coverage(N, *byname[name], sx, sy)
        tot = inp.channel_sums(S)[0]
        D = inp.observe(cube, S, weighting)
        if D.any():
            assert np.max(np.abs(D.imag)) <= 1e-13 * np.max(np.abs(D)), name
        assert not D[:, :, tot == 0].any(), name
        P = inp.psf(S, weighting)
        assert np.allclose(P[0, 0, tot > 0], 1., rtol=0, atol=1e-13) and not P[:, :, tot == 0].any(), name


@pytest.mark.parametrize("geom", GEOMS)
def test_uniform_weighting_of_full_coverage_is_the_identity(geom):
    N, sx, sy = ic.tables(geom)
    S = inp.coverage(N, ic.everywhere_set(N, sx, sy), None, sx, sy)
    cube = ic.smooth_cube(N)
    D = inp.observe(cube, S, "uniform")
    assert np.max(np.abs(D - cube)) <= 1e-13 * np.max(np.abs(cube))
    beam = 1. / (1. + np.arange(N)[:, None, None] * 0.1) * np.ones((N, N, N))
    D = inp.observe(cube, S, "uniform", beam=beam)
    assert np.max(np.abs(D - beam * cube)) <= 1e-13 * np.max(np.abs(cube))


@pytest.mark.parametrize("geom", GEOMS)
def test_noise_variance_is_sigma2_over_tot(geom):
    """Deterministic: white unit g has the identity as covariance, so the variance of pixel p of the noise cube is the sum of
    squares of the operator's response to an impulse (the operator is a circular convolution: any pixel gives the same)."""
    N, sx, sy = ic.tables(geom)
    byname = {name: (s, m) for name, s, m in ic.cases(N, sx, sy)}
    sigma = np.linspace(0.5, 2., N)
    for name in ("random1000", "band-edge", "copies-collapsed"):
        S = inp.coverage(N, *byname[name], sx, sy)
        tot = inp.channel_sums(S)[0]
        ok = tot > 0
        for at in ((0, 0), (3, N - 2)):
            h = inp.noise(inp.impulse(N, at), S, 1.)
            assert np.allclose(np.sum(np.abs(h) ** 2, axis=(0, 1))[ok], 1. / tot[ok], rtol=1e-12), name
            h = inp.noise(inp.impulse(N, at), S, sigma)
            assert np.allclose(np.sum(np.abs(h) ** 2, axis=(0, 1))[ok], sigma[ok] ** 2 / tot[ok], rtol=1e-12), name
            assert np.max(np.abs(h.imag)) <= 1e-13 * np.max(np.abs(h)) and not h[:, :, ~ok].any(), name


def test_weight_statement_rounds_once():
    N = 16
    rs = np.random.RandomState(2)
    spec = (rs.normal(size=(N, N, N)) + 1j * rs.normal(size=(N, N, N)))
    S = rs.randint(0, 50, (N, N, N)).astype(np.int32)
    scale = rs.uniform(0.1, 3., N)
    for mode in (inp.NATURAL, inp.UNIFORM, inp.SQRT):
        fac = inp.factor(S, mode, scale)
        w64 = inp.weight(spec, S, mode, scale)
        assert w64.dtype == np.complex128 and np.array_equal(w64.real, spec.real * fac) and np.array_equal(w64.imag, spec.imag * fac)
        w32 = inp.weight(spec.astype(np.complex64), S, mode, scale)
        assert w32.dtype == np.complex64
        assert np.array_equal(w32.real, (spec.real.astype(np.float32).astype(np.float64) * fac).astype(np.float32))
    assert np.array_equal(inp.factor(S, inp.UNIFORM, np.ones(N)), (S > 0) * 1.)


def test_constructor_checks_need_no_device():
    """The sample checks of Interferometer run before anything touches the device: a host stand-in for the box is enough."""
    hb = ic.HostBox(16, 1e3)
    with pytest.raises(ValueError):
        itf.Interferometer(hb, baselines=[[1., np.nan]])
    with pytest.raises(ValueError):
        itf.Interferometer(hb, baselines=[[np.inf, 0.]])
    with pytest.raises(ValueError):
        itf.Interferometer(hb, baselines=[[1., 2.]], multiplicity=[2 ** 30])           # 2 sum(m) = 2^31 > 2^31 - 1
    with pytest.raises(ValueError):
        itf.Interferometer(hb)
    with pytest.raises(ValueError):
        itf.Interferometer(hb, baselines=[[1., 2.]], latitude=0.1)
    ok = itf.Interferometer(hb, baselines=[[1., 2.]], multiplicity=[2 ** 30 - 1])
    assert ok.uv_samples().shape == (1, 2)
    inst = itf.Interferometer(hb, antennas=itf.hex_array(3, 10.), latitude=-0.5, declination=-0.4, hour_angles=[-0.1, 0., 0.1])
    assert inst.uv_samples().shape == (19 * 18 // 2 * 3, 2)
    uniq, mult = inst._collapsed()
    assert mult.sum() == inst.uv_samples().shape[0] and mult.dtype == np.int32
