"""GPU: CosmoBox.power_spectrum and its C entries (fb_bin_power_kmu, fb_power_spectrum_kmu) against the numpy statement of
the definition (tests/pk_numpy.py) computed on the values the plan holds; agreement with binned_power_spectrum, identities,
lazy inputs, the box's state, argument errors, a 1024^3 default call and a Kaiser-factor physics check."""
import time

import numpy as np
import pytest

from fastbox_amd import BeamHighpass, CosmoBox, default_cosmo, hostgeom
from tests import pk_numpy as pk

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


def _close_rel(a, b, rel):
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def _compare(box, d1, d2, edges, mode, Nmu, poles, prec, label=""):
    h1 = _stored(d1, prec)
    h2 = None if d2 is None else _stored(d2, prec)
    kw = dict(delta_x=d1, second=d2, mode=mode, Nmu=Nmu, poles=poles)
    if edges is not None:
        kw["kbins"] = edges
    got = box.power_spectrum(**kw)
    e = hostgeom.power_edges(_L(box), box.N) if edges is None else np.asarray(edges, dtype=np.float64)
    ref = pk.power_spectrum(h1, h2, _L(box), e, mode=mode, Nmu=Nmu, poles=None if poles is None else list(poles))
    nk = e.size - 1
    for a in got:
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.writeable
    if mode == "2d":
        k, mu, p, n = got
        ok_, omu, op, on = ref
        assert k.shape == mu.shape == p.shape == n.shape == (nk, Nmu)
        pairs = [(k, ok_), (mu, omu)]
    else:
        k, p, n = got
        ok_, op, on = ref
        assert k.shape == n.shape == (nk,)
        assert p.shape == ((nk,) if poles is None else (len(poles), nk))
        pairs = [(k, ok_)]
    assert np.array_equal(n, on), "modes differ"
    m = on > 0
    for a, b in pairs:
        assert np.array_equal(np.isnan(a), ~m)
        assert _close_rel(a[m], b[m], 1e-14)
    if mode == "2d" or poles is None:
        assert np.array_equal(np.isnan(p), ~m)
        pm, opm = p[m], op[m]
    else:
        assert np.all(np.isnan(p[:, ~m])) and not np.any(np.isnan(p[:, m]))
        pm, opm = p[:, m], op[:, m]
    scale = np.max(np.abs(opm)) if opm.size else 1.
    dev = np.max(np.abs(pm - opm)) / scale if opm.size else 0.
    print("power %s N=%d %s %s %s Nmu=%d poles=%s nk=%d: modes equal; max |d P| / max |P| = %.3e"
          % (label, box.N, prec, "cross" if d2 is not None else "auto", mode, Nmu if mode == "2d" else 1, poles, nk, dev))
    assert dev <= TOL[prec]
    return got


def _edges(box, bins):
    kf = 2. * np.pi / min(_L(box))
    if bins == "default":
        return None
    if bins == "shells":                       # edges exactly on |k| of axis-aligned modes
        return np.arange(0., 0.4 * box.N * kf, kf)
    if bins == "between":                      # edges between the shells of a cube
        return np.arange(0.5 * kf, 0.5 * box.N * kf, kf)
    return np.geomspace(kf, 0.5 * box.N * kf, 17)        # "log": non-uniform edges


CASES = [
    # N, L, prec, cross, bins, mode, Nmu, poles
    (16, 1e2, "f64", False, "default", "1d", 5, None),
    (16, (1e2, 2e2, 1e3), "f32", True, "shells", "2d", 4, None),
    (32, 1e3, "f64", True, "default", "1d", 5, [0, 2, 4]),
    (32, 1e3, "f32", False, "log", "2d", 5, None),
    (48, 1e3, "f64", True, "default", "2d", 5, None),
    (48, 1e3, "f32", False, "shells", "1d", 5, [0, 2, 4]),
    (64, (1e2, 2e2, 1e3), "f64", False, "default", "1d", 5, [2, 4]),
    (64, 1e3, "f32", True, "between", "2d", 10, None),
    (128, 1e3, "f64", False, "shells", "2d", 5, None),
    (128, (1e2, 2e2, 1e3), "f32", True, "default", "1d", 5, [0, 2, 4]),
    (256, 1e3, "f32", False, "default", "2d", 5, None),
    (256, 1e3, "f64", True, "default", "1d", 5, [0, 2, 4]),
    (512, 1e3, "f32", False, "default", "1d", 5, [0, 2, 4]),
]


@pytest.mark.parametrize("N,L,prec,cross,bins,mode,Nmu,poles", CASES)
def test_against_numpy(N, L, prec, cross, bins, mode, Nmu, poles):
    box = _box(N, L, prec)
    d1, d2 = _fields(box, cross)
    _compare(box, d1, d2, _edges(box, bins), mode, Nmu, poles, prec, label=bins)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [32, 128])
def test_auto_equals_binned_power_spectrum(prec, N):
    box = _box(N, 1e3, prec)
    d = box.realise_density(inplace=False)
    edges = _edges(box, "between")[:200]
    k, p, n = box.power_spectrum(delta_x=d, kbins=edges)
    kc, pb, err = box.binned_power_spectrum(delta_x=d, kbins=edges)
    m = n > 0
    assert np.array_equal(np.isnan(pb), ~m)
    dev = np.max(np.abs(p[m] - pb[m])) / np.max(np.abs(pb[m]))
    print("power vs binned_power_spectrum N=%d %s: max |d P| / max |P| = %.3e" % (N, prec, dev))
    assert dev <= TOL[prec]


def test_halo_matter_cross_equals_difference_of_autos():
    N, L = 64, 500.
    box = _box(N, L, "f64")
    d = np.asarray(box.realise_density(inplace=False))
    rs = np.random.RandomState(3)
    pos = rs.uniform(0., L, (60000, 3))
    mesh = box.paint_catalogue(pos, window="cic")
    h = np.asarray(mesh) / (60000. / N ** 3) - 1.
    edges = _edges(box, "between")
    k, pc, n = box.power_spectrum(delta_x=mesh, second=d, kbins=edges)
    pmesh = box.power_spectrum(delta_x=h, second=d, kbins=edges)[1]
    p_sum = box.binned_power_spectrum(delta_x=h + d, kbins=edges)[1]
    p_h = box.binned_power_spectrum(delta_x=h, kbins=edges)[1]
    p_d = box.binned_power_spectrum(delta_x=d, kbins=edges)[1]
    diff = 0.5 * (p_sum - p_h - p_d)
    m = n > 0
    # the mesh itself and its overdensity differ by a factor and the mean (k = 0 only)
    assert np.allclose(pc[m] * N ** 3 / 60000., pmesh[m], rtol=1e-12, atol=0)
    dev = np.max(np.abs(pmesh[m] - diff[m])) / np.max(p_h[m] + p_d[m])
    print("power halo x matter vs (P(h+d) - P(h) - P(d)) / 2: max dev / max(P_h + P_d) = %.3e" % dev)
    assert dev <= 1e-11


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_identities(prec):
    box = _box(64, (1e3, 1e3, 2e3), prec)
    a, b = _fields(box, True)
    kw = dict(poles=[0, 2, 4])
    tol = TOL[prec]
    auto = box.power_spectrum(delta_x=a, **kw)
    same = box.power_spectrum(delta_x=a, second=a, **kw)
    assert np.array_equal(auto[2], same[2])
    assert np.nanmax(np.abs(auto[1] - same[1])) <= tol * np.nanmax(np.abs(auto[1]))
    ab = box.power_spectrum(delta_x=a, second=b, **kw)
    ba = box.power_spectrum(delta_x=b, second=a, **kw)
    assert np.nanmax(np.abs(ab[1] - ba[1])) <= tol * np.nanmax(np.abs(ab[1]))
    # the mu-summed 2-d power with modes as weights is the 1-d power
    k2, mu2, p2, n2 = box.power_spectrum(delta_x=a, second=b, mode="2d", Nmu=7)
    k1, p1, n1 = box.power_spectrum(delta_x=a, second=b)
    assert np.array_equal(n2.sum(axis=1), n1)
    m = n1 > 0
    p_from_2d = np.nansum(p2 * n2, axis=1)[m] / n1[m]
    k_from_2d = np.nansum(k2 * n2, axis=1)[m] / n1[m]
    assert np.max(np.abs(p_from_2d - p1[m])) <= tol * np.max(np.abs(p1[m]))
    assert _close_rel(k_from_2d, k1[m], 1e-13)
    # two calls are bit-identical
    again = box.power_spectrum(delta_x=a, second=b, mode="2d", Nmu=7)
    for x, y in zip((k2, mu2, p2, n2), again):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bin_geometry_is_recomputed_after_eviction(prec):
    """The plan keeps the data-independent sums (modes, mean |k|, mean mu per cell) of the last 16 (edges, Nmu) sets: after 17
    other sets the first one is computed again, and the whole result is what it was (NaN where a cell holds no mode)."""
    box = _box(32, 1e3, prec)
    d1 = box.realise_density(inplace=False)
    kf = 2. * np.pi / 1e3
    first = box.power_spectrum(delta_x=d1, mode="2d", kbins=np.arange(0.5 * kf, 16. * kf, kf), Nmu=5)
    for q in range(17):                        # 17 distinct sets: the edges differ in all of them, Nmu in most
        box.power_spectrum(delta_x=d1, mode="2d", kbins=np.arange(0.5 * kf, 16. * kf, (1.1 + 0.05 * q) * kf), Nmu=3 + q % 5)
    again = box.power_spectrum(delta_x=d1, mode="2d", kbins=np.arange(0.5 * kf, 16. * kf, kf), Nmu=5)
    assert first[3].sum() > 0 and np.array_equal(first[3], again[3])
    for x, y in zip(first, again):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lazy_inputs_equal_materialised(prec):
    box = _box(64, 1e3, prec)                  # (64: the size from which f32 boxes defer the redshift-space remap)
    kw = dict(mode="2d", Nmu=4)

    def same(lazy, label, second=None):
        a = box.power_spectrum(delta_x=lazy, second=second, **kw)
        b = box.power_spectrum(delta_x=np.asarray(lazy), second=None if second is None else np.asarray(second), **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), label
    dx = box.realise_density()                 # device generator: the last FFT pass still pending
    same(dx, "realise_density")
    dx2 = box.realise_density()
    same(box.lognormal(dx2), "lognormal")
    box.realise_density()
    box.realise_velocity()
    vz = box.to_real(box.velocity_k[2])
    same(box.redshift_space_density(delta_x=box.delta_x, velocity_z=vz, sigma_nl=0.), "redshift_space_density")
    filt = BeamHighpass(kpar0=0.05, kperp0=0.3)
    same(box.apply_transfer_fn(box.to_k(box.delta_x), filt).real, "apply_transfer_fn")
    rs = np.random.RandomState(1)
    same(box.paint_catalogue(rs.uniform(0., 1e3, (5000, 3)), window="tsc"), "paint_catalogue")
    dx3 = box.realise_density(inplace=False)
    same(dx2, "cross", second=dx3)


def test_box_state_is_untouched():
    box = _box(32, 1e3, "f32")
    box.realise_density()
    before = box.binned_power_spectrum()
    dx, counter, cache = box.delta_x, box._realisation, dict(box._bin_cache)
    one = box.power_spectrum(poles=[0, 2, 4])
    two = box.power_spectrum(poles=[0, 2, 4])
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)
    box.power_spectrum(mode="2d")
    assert box._realisation == counter and box.delta_x is dx and box._delta_k is None
    assert box._bin_cache.keys() == cache.keys()
    after = box.binned_power_spectrum()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)


def test_argument_errors_before_device_work():
    box = _box(16, 1e2, "f32")
    box.realise_density()
    pool = {k: list(v) for k, v in box.engine._pool.items()}
    bad = [dict(second=np.zeros((8, 8, 8))), dict(kbins=[0., 0.5, 0.3]), dict(kbins=[-0.1, 0.5]), dict(poles=[1]),
           dict(mode="3d"), dict(mode="2d", poles=[0]), dict(mode="2d", Nmu=0), dict(mode="2d", Nmu=129),
           dict(kbins=np.linspace(0., 10., 1026)), dict(mode="2d", Nmu=6, kbins=np.linspace(0., 10., 1025))]
    for kw in bad:
        with pytest.raises(ValueError):
            box.power_spectrum(**kw)
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool
    other = _box(16, 1e2, "f32")
    with pytest.raises(ValueError):
        box.power_spectrum(second=other.realise_density())


def test_c_entries():
    from fastbox_amd import _lib
    lib = _lib.load()
    assert lib.fb_version() >= 102
    for name in ("fb_bin_power_kmu", "fb_power_spectrum_kmu"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    box = _box(32, 1e3, "f64")
    eng = box.engine
    d1 = box.realise_density(inplace=False)
    d2 = box.realise_density(inplace=False)
    edges = np.arange(0., 0.1, 2. * np.pi / 1e3)
    nk, nmu, lmax = edges.size - 1, 3, 4
    ep = edges.ctypes.data_as(_lib.P_double)
    one = np.zeros(4 * nk * nmu + 2 * nk)
    wh1, wh2 = eng.empty("half"), eng.empty("half")
    assert lib.fb_power_spectrum_kmu(eng._plan, d1.ptr, d2.ptr, wh1.ptr, wh2.ptr, ep, nk, nmu, lmax,
                                     one.ctypes.data_as(_lib.P_double), eng.stream) == 0
    # the binning entry on transforms made separately gives the same record
    h1, h2 = eng.fft_r2c(d1), eng.fft_r2c(d2)
    two = np.zeros_like(one)
    _lib.call("fb_bin_power_kmu", eng._plan, h1.ptr, h2.ptr, ep, nk, nmu, lmax, two.ctypes.data_as(_lib.P_double), eng.stream)
    assert np.array_equal(one, two)
    # against the restatement: modes per cell, and the per-k sums of P L_l over the mu cells
    s = pk.power_sums(np.asarray(d1), np.asarray(d2), _L(box), edges, Nmu=nmu, lmax=lmax)
    nc = nk * nmu
    assert np.array_equal(one[:nc], s["modes"].ravel())
    ps = np.max(np.abs(s["sum_p"]))
    assert np.max(np.abs(one[3 * nc:4 * nc] - s["sum_p"].ravel())) <= 1e-11 * ps
    for q, l in enumerate((2, 4)):
        assert np.max(np.abs(one[4 * nc + q * nk:4 * nc + (q + 1) * nk] - s["sum_pl"][l].sum(axis=1))) <= 1e-11 * ps
    # invalid arguments
    out = np.zeros(8 * 1024 * 5 + 4096)
    o = out.ctypes.data_as(_lib.P_double)

    def e(*v):
        a = np.array(v, dtype=np.float64)
        return a, a.ctypes.data_as(_lib.P_double)
    good = e(0., 0.05, 0.1)
    big = e(*np.linspace(0., 1., 1026))
    for arr, k_, mu_, l_ in [(e(0., 0.05, 0.05), 2, 1, 0), (e(0., 0.05, 0.01), 2, 1, 0), (e(-1., 0.05, 0.1), 2, 1, 0),
                             (good, 0, 1, 0), (good, 2, 0, 0), (good, 2, 129, 0), (good, 2, 1, 1), (good, 2, 1, 6),
                             (big, 1025, 1, 0), (e(*np.linspace(0., 1., 1025)), 1024, 5, 2), (e(0., np.nan, 0.1), 2, 1, 0)]:
        assert lib.fb_bin_power_kmu(eng._plan, h1.ptr, None, arr[1], k_, mu_, l_, o, eng.stream) == -1
        assert lib.fb_power_spectrum_kmu(eng._plan, d1.ptr, None, wh1.ptr, None, arr[1], k_, mu_, l_, o, eng.stream) == -1
    assert lib.fb_power_spectrum_kmu(eng._plan, d1.ptr, d2.ptr, wh1.ptr, None, good[1], 2, 1, 0, o, eng.stream) == -1
    assert lib.fb_bin_power_kmu(eng._plan, None, None, good[1], 2, 1, 0, o, eng.stream) == -1
    assert lib.fb_bin_power_kmu(eng._plan, h1.ptr, None, good[1], 2, 1, 0, None, eng.stream) == -1
    # the largest layouts are accepted: 1024 x 5 cells, and 1024 k bins with three multipoles
    full = e(*np.linspace(0., 0.4, 1025))
    assert lib.fb_bin_power_kmu(eng._plan, h1.ptr, None, full[1], 1024, 5, 0, o, eng.stream) == 0
    assert out[:5120].sum() > 0
    assert lib.fb_bin_power_kmu(eng._plan, h1.ptr, None, full[1], 1024, 1, 4, o, eng.stream) == 0


def test_default_edges_at_1024():
    """One default call of each mode on a 1024^3 f32 box: 512 k bins (5 x 512 cells in 2-d).  modes against a host count."""
    N, L = 1024, 1e3
    box = _box(N, L, "f32")
    box.realise_density()
    t0 = time.perf_counter()
    k1, p1, n1 = box.power_spectrum()
    t1 = time.perf_counter()
    k2, mu2, p2, n2 = box.power_spectrum(mode="2d")
    t2 = time.perf_counter()
    kp, pp, np_ = box.power_spectrum(poles=[0, 2, 4])
    t3 = time.perf_counter()
    k2b, mu2b, p2b, n2b = box.power_spectrum(mode="2d")
    t4 = time.perf_counter()
    assert n1.shape == (512,) and n2.shape == (512, 5) and pp.shape == (3, 512)
    edges = hostgeom.power_edges((L, L, L), N)
    kx = pk.wavenumbers(N, (L, L, L))[0]
    l = np.arange(N // 2 + 1)
    kz = kx[l]
    w = np.where((l == 0) | (l == N // 2), 1., 2.)
    host = np.zeros(512 * 5)
    for i in range(N):
        K = np.sqrt((kx[i] * kx[i] + kx[:, None] * kx[:, None]) + kz[None, :] * kz[None, :])
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = np.where(K > 0, np.abs(kz)[None, :] / K, 0.)
        cell, ok = pk._bin_cells(K, mu, edges, 5)
        host += np.bincount(cell[ok], weights=np.broadcast_to(w, K.shape)[ok], minlength=512 * 5)
    assert np.array_equal(n2.ravel(), host)
    assert np.array_equal(n1, host.reshape(512, 5).sum(axis=1)) and np.array_equal(np_, n1)
    m = n1 > 0
    assert np.max(np.abs(p1[m] - pp[0][m])) <= 1e-12 * np.max(p1[m]) and np.all(p1[m] > 0)
    assert np.max(np.abs(np.nansum(p2 * n2, axis=1)[m] / n1[m] - p1[m])) <= 1e-12 * np.max(p1[m])
    print("power default edges N=1024 f32: 1d %.1f ms, 2d %.1f ms (first: geometry pass), poles %.1f ms, 2d again %.1f ms"
          % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t4 - t3)))


def test_kaiser_quadrupole():
    """A spectrum multiplied by the Kaiser factor (1 + beta mu^2)^2 (the field by 1 + beta mu^2, through apply_transfer_fn):
    P_2 / P_0 -> (4 beta/3 + 4 beta^2/7) / (1 + 2 beta/3 + beta^2/5) on large scales."""
    N, L, beta = 128, 1e3, 0.5
    box = _box(N, L, "f64")
    box.realise_density()
    kaiser = lambda kperp, kpar: 1. + beta * kpar ** 2 / (kperp ** 2 + kpar ** 2)     # the field's factor: P gets its square
    field = box.apply_transfer_fn(box.to_k(box.delta_x), kaiser).real
    kf = 2. * np.pi / L
    edges = np.arange(0.5 * kf, 12.5 * kf, kf)                          # large scales: 12 shells
    k, p, n = box.power_spectrum(delta_x=field, kbins=edges, poles=[0, 2])
    ratio = np.sum(p[1] * n) / np.sum(p[0] * n)
    expect = (4. * beta / 3. + 4. * beta ** 2 / 7.) / (1. + 2. * beta / 3. + beta ** 2 / 5.)
    # the Gaussian field's scatter: P_2 / P_0 of n modes has an rms of about sqrt(5 * 2 / n) relative to P_0
    tol = 4. * np.sqrt(10. / n.sum())
    print("power Kaiser beta=%.2f N=%d: P2/P0 = %.4f, expected %.4f, tolerance %.4f (%d modes)"
          % (beta, N, ratio, expect, tol, n.sum()))
    assert abs(ratio - expect) <= tol
