"""GPU: CosmoBox.cylindrical_power_spectrum and its C entries (fb_bin_power_cyl, fb_power_spectrum_cyl) against the numpy
statement of the definition (tests/cyl_numpy.py) computed on the values the plan holds: auto and cross, both precisions, grids
that are and are not powers of two, a cuboid, default edges, edges on mode values, an inf edge, dropped modes, an empty cell, a
single bin, lazy inputs, the box's state, repeatability, argument errors, and agreement with power_spectrum(mode='1d').
Tolerances are those of tests/test_power_spectrum_gpu.py."""
import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, hostgeom
from tests import cyl_numpy as cn

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-5}          # |d P| <= TOL * max |P| of the call


def _box(N, L, prec, rng="device", seed=7):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng=rng, seed=seed)


def _stored(x, prec):
    """The values a plan of this precision holds for a host field."""
    return np.asarray(x, dtype=np.float64).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)


def _fields(box, cross):
    d1 = np.asarray(box.realise_density(inplace=False))
    d2 = 0.6 * d1 + np.asarray(box.realise_density(inplace=False)) if cross else None
    return d1, d2


def _L(box):
    return (box.Lx, box.Ly, box.Lz)


def _compare(box, d1, d2, perp, par, prec, label=""):
    kw = dict(delta_x=d1, second=d2)
    if perp is not None:
        kw["kperp_bins"] = perp
    if par is not None:
        kw["kpar_bins"] = par
    got = box.cylindrical_power_spectrum(**kw)
    dpe, dqe = hostgeom.cyl_edges(_L(box), box.N)
    pe = dpe if perp is None else np.asarray(perp, dtype=np.float64)
    qe = dqe if par is None else np.asarray(par, dtype=np.float64)
    ref = cn.cylindrical_power_spectrum(_stored(d1, prec), None if d2 is None else _stored(d2, prec), _L(box), pe, qe)
    for a in got:
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.writeable
        assert a.shape == (pe.size - 1, qe.size - 1)
    kperp, kpar, p, n = got
    okperp, okpar, op, on = ref
    assert np.array_equal(n, on), "modes differ"
    m = on > 0
    for a, b in ((kperp, okperp), (kpar, okpar)):
        assert np.array_equal(np.isnan(a), ~m)
        assert np.all(np.abs(a[m] - b[m]) <= 1e-14 * np.abs(b[m]))
    assert np.array_equal(np.isnan(p), ~m)
    scale = np.max(np.abs(op[m])) if m.any() else 1.
    dev = np.max(np.abs(p[m] - op[m])) / scale if m.any() else 0.
    print("cylindrical %s N=%d %s %s cells=%dx%d: modes equal; max |d P| / max |P| = %.3e"
          % (label, box.N, prec, "cross" if d2 is not None else "auto", pe.size - 1, qe.size - 1, dev))
    assert dev <= TOL[prec]
    return got


def _edges(box, bins):
    """(k_perp edges, k_par edges); None: the defaults."""
    Lx, Ly, Lz = _L(box)
    N = box.N
    kf, kz = 2. * np.pi / min(Lx, Ly), 2. * np.pi / Lz
    if bins == "default":
        return None, None
    if bins == "on_modes":                     # edges exactly on mode values: a mode on an edge belongs to the upper bin
        return np.arange(0., 0.5 * N) * kf, np.arange(0., N // 2 + 2) * kz
    if bins == "inf":                          # a last edge of inf on both axes, uneven edges
        return np.array([0., 0.8 * kf, 2.3 * kf, 5.1 * kf, np.inf]), np.array([-0.5 * kz, 1.5 * kz, 4.2 * kz, np.inf])
    if bins == "dropped":                      # modes dropped below the first and above the last edge, on both axes
        return np.arange(1.5, 0.3 * N, 0.75) * kf, np.arange(0.5, 0.35 * N, 1.5) * kz
    if bins == "empty":                        # (1.05, 1.35) kf holds no k_perp (1 and sqrt(2) are neighbours): empty cells
        return np.array([0., 1.05 * kf, 1.35 * kf, 3. * kf]), np.array([-0.5 * kz, 0.2 * kz, 0.8 * kz, 3.5 * kz])
    assert bins == "single"
    return np.array([0., np.inf]), np.array([-1., np.inf])


CASES = [
    # N, L, prec, cross, bins
    (16, 1e2, "f64", False, "default"),
    (16, 1e2, "f32", True, "on_modes"),
    (16, (1e2, 2e2, 1e3), "f64", True, "default"),
    (16, (1e2, 2e2, 1e3), "f32", False, "on_modes"),
    (16, 1e2, "f64", False, "empty"),
    (24, 1e3, "f64", True, "default"),
    (24, 1e3, "f32", False, "inf"),
    (24, 1e3, "f64", False, "dropped"),
    (64, 1e3, "f64", False, "default"),
    (64, 1e3, "f32", True, "default"),
    (64, 1e3, "f32", False, "on_modes"),
    (64, 1e3, "f64", True, "inf"),
    (64, (1e3, 2e3, 5e2), "f64", False, "dropped"),
    (64, 1e3, "f32", False, "single"),
    (16, 1e2, "f64", True, "single"),
    (128, 1e3, "f32", False, "default"),
]


@pytest.mark.parametrize("N,L,prec,cross,bins", CASES)
def test_against_numpy(N, L, prec, cross, bins):
    box = _box(N, L, prec)
    d1, d2 = _fields(box, cross)
    perp, par = _edges(box, bins)
    kperp, kpar, p, n = _compare(box, d1, d2, perp, par, prec, label=bins)
    if bins == "empty":
        assert np.all(n[1] == 0) and np.all(np.isnan(p[1])) and np.all(n[:, 1] == 0) and np.all(np.isnan(p[:, 1]))
        assert np.all(n[[0, 2]][:, [0, 2]] > 0)
    if bins == "single":
        assert n.shape == (1, 1) and n[0, 0] == N ** 3 - 1
    if bins == "on_modes" and np.isscalar(L):
        # a mode on an edge is in the upper bin: k = 0 excluded; (0, 0, +-1); (+-1, 0, 0), (0, +-1, 0), (+-1, +-1, 0)
        assert n[0, 0] == 0 and n[0, 1] == 2 and n[1, 0] == 8 and n[0, N // 2] == 1 and n[1, 1] == 16


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [16, 64])
def test_single_cell_equals_power_spectrum_1d(prec, N):
    """Edges for which every cylindrical cell falls inside one |k| shell: one k_perp bin and one k_par bin against one k bin."""
    box = _box(N, 1e3, prec)
    a, b = _fields(box, True)
    kperp, kpar, p, n = box.cylindrical_power_spectrum(delta_x=a, second=b, kperp_bins=[0., np.inf], kpar_bins=[-1., np.inf])
    k1, p1, n1 = box.power_spectrum(delta_x=a, second=b, kbins=[0., np.inf])
    assert n[0, 0] == n1[0] == N ** 3 - 1
    assert abs(p[0, 0] - p1[0]) <= TOL[prec] * abs(p1[0])
    # several cells summed into the same shell with modes as weights
    kf = 2. * np.pi / 1e3
    k2, q2, p2, n2 = box.cylindrical_power_spectrum(delta_x=a, second=b, kperp_bins=[0., 2.2 * kf, 5.7 * kf, np.inf],
                                                    kpar_bins=[-1., 0.5 * kf, 3.5 * kf, np.inf])
    assert n2.sum() == n1[0]
    assert abs(np.sum(p2 * n2) / n2.sum() - p1[0]) <= TOL[prec] * abs(p1[0])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lazy_and_host_inputs_and_repeatability(prec):
    box = _box(64, 1e3, prec)

    def same(lazy, label, second=None):
        a = box.cylindrical_power_spectrum(delta_x=lazy, second=second)
        b = box.cylindrical_power_spectrum(delta_x=np.asarray(lazy), second=None if second is None else np.asarray(second))
        c = box.cylindrical_power_spectrum(delta_x=lazy, second=second)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y, equal_nan=True), label
            assert np.array_equal(x, z, equal_nan=True), label + ": two calls differ"
    dx = box.realise_density()                 # device generator: the last FFT pass still pending
    same(dx, "realise_density")
    dx2 = box.realise_density()
    same(box.lognormal(dx2), "lognormal")
    dx3 = box.realise_density(inplace=False)
    same(dx2, "cross", second=dx3)
    box.realise_density()
    auto = box.cylindrical_power_spectrum()    # the box's own delta_x
    again = box.cylindrical_power_spectrum(delta_x=box.delta_x)
    for x, y in zip(auto, again):
        assert np.array_equal(x, y, equal_nan=True)


def test_box_state_is_untouched():
    box = _box(32, 1e3, "f32")
    box.realise_density()
    before = box.binned_power_spectrum()
    dx, counter, cache = box.delta_x, box._realisation, dict(box._bin_cache)
    one = box.cylindrical_power_spectrum()
    two = box.cylindrical_power_spectrum()
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)
    box.cylindrical_power_spectrum(kperp_bins=[0., 0.05, 0.2])
    assert box._realisation == counter and box.delta_x is dx and box._delta_k is None
    assert box._bin_cache.keys() == cache.keys()
    after = box.binned_power_spectrum()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)


def test_argument_errors_before_device_work():
    box = _box(16, 1e2, "f32")
    box.realise_density()
    pool = {k: list(v) for k, v in box.engine._pool.items()}
    bad = [dict(second=np.zeros((8, 8, 8))), dict(delta_x=np.zeros((16, 16))), dict(kperp_bins=[0., 0.5, 0.3]),
           dict(kperp_bins=[-0.1, 0.5]), dict(kperp_bins=[0.3]), dict(kpar_bins=[0., 0.5, 0.5]), dict(kpar_bins=[0., np.nan]),
           dict(dk_perp=0.), dict(kperp_bins=np.linspace(0., 10., 1026)), dict(kpar_bins=np.linspace(0., 10., 1027))]
    for kw in bad:
        with pytest.raises(ValueError):
            box.cylindrical_power_spectrum(**kw)
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool
    other = _box(16, 1e2, "f32")
    with pytest.raises(ValueError):
        box.cylindrical_power_spectrum(second=other.realise_density())
    with pytest.raises(ValueError):
        _box(16, 1e2, "f32").cylindrical_power_spectrum()          # no delta_x yet


def test_c_entries():
    from fastbox_amd import _lib
    lib = _lib.load()
    box = _box(24, (1e3, 2e3, 5e2), "f64")
    eng = box.engine
    d1 = box.realise_density(inplace=False)
    d2 = box.realise_density(inplace=False)
    pe = np.arange(0., 0.07, 2. * np.pi / 1e3)
    qe = np.array([-0.01, 0.02, 0.05, 0.11, np.inf])
    nperp, npar = pe.size - 1, qe.size - 1
    pp, qp = pe.ctypes.data_as(_lib.P_double), qe.ctypes.data_as(_lib.P_double)
    one = np.zeros(4 * nperp * npar)
    wh1, wh2 = eng.empty("half"), eng.empty("half")
    assert lib.fb_power_spectrum_cyl(eng._plan, d1.ptr, d2.ptr, wh1.ptr, wh2.ptr, pp, nperp, qp, npar,
                                     one.ctypes.data_as(_lib.P_double), eng.stream) == 0
    # the binning entry on transforms made separately gives the same record
    h1, h2 = eng.fft_r2c(d1), eng.fft_r2c(d2)
    two = np.zeros_like(one)
    _lib.call("fb_bin_power_cyl", eng._plan, h1.ptr, h2.ptr, pp, nperp, qp, npar, two.ctypes.data_as(_lib.P_double), eng.stream)
    assert np.array_equal(one, two)
    s = cn.cyl_sums(np.asarray(d1), np.asarray(d2), _L(box), pe, qe)
    nc = nperp * npar
    assert np.array_equal(one[:nc], s["modes"].ravel())
    for q, key in ((1, "sum_kperp"), (2, "sum_kpar")):
        assert np.all(np.abs(one[q * nc:(q + 1) * nc] - s[key].ravel()) <= 1e-14 * np.abs(s[key].ravel()))
    assert np.max(np.abs(one[3 * nc:] - s["sum_p"].ravel())) <= 1e-11 * np.max(np.abs(s["sum_p"]))
    # invalid arguments
    out = np.zeros(4 * 1024 * 4)
    o = out.ctypes.data_as(_lib.P_double)

    def e(*v):
        a = np.array(v, dtype=np.float64)
        return a, a.ctypes.data_as(_lib.P_double)
    good, gpar = e(0., 0.05, 0.1), e(-0.01, 0.05, np.inf)
    for pa, n1, qa, n2 in [(e(0., 0.05, 0.05), 2, gpar, 2), (e(-1., 0.05, 0.1), 2, gpar, 2), (e(0., np.nan, 0.1), 2, gpar, 2),
                           (good, 0, gpar, 2), (good, 1025, gpar, 2), (good, 2, gpar, 0), (good, 2, gpar, 1026),
                           (good, 2, e(0., 0.05, 0.01), 2), (good, 2, e(0., np.inf, np.inf), 2)]:
        assert lib.fb_bin_power_cyl(eng._plan, h1.ptr, None, pa[1], n1, qa[1], n2, o, eng.stream) == -1
        assert lib.fb_power_spectrum_cyl(eng._plan, d1.ptr, None, wh1.ptr, None, pa[1], n1, qa[1], n2, o, eng.stream) == -1
    assert lib.fb_power_spectrum_cyl(eng._plan, d1.ptr, d2.ptr, wh1.ptr, None, good[1], 2, gpar[1], 2, o, eng.stream) == -1
    assert lib.fb_bin_power_cyl(eng._plan, None, None, good[1], 2, gpar[1], 2, o, eng.stream) == -1
    # the largest k_perp layout is accepted; more edge sets than the plan keeps are served
    full = e(*np.linspace(0., 0.4, 1025))
    assert lib.fb_bin_power_cyl(eng._plan, h1.ptr, None, full[1], 1024, gpar[1], 2, o, eng.stream) == 0
    assert out[:2048].sum() > 0
    for q in range(10):
        sh = e(0., 0.01 + 0.001 * q, 0.1)
        assert lib.fb_bin_power_cyl(eng._plan, h1.ptr, None, sh[1], 2, gpar[1], 2, o, eng.stream) == 0
    three = np.zeros_like(one)
    _lib.call("fb_bin_power_cyl", eng._plan, h1.ptr, h2.ptr, pp, nperp, qp, npar, three.ctypes.data_as(_lib.P_double), eng.stream)
    assert np.array_equal(one, three)
