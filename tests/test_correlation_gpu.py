"""GPU: CosmoBox.correlation_function and its C entries (fb_cross_power_half, fb_bin_separation,
fb_correlation_function) against the numpy statement of the definition (tests/corrfn_numpy.py): brute force at 16^3,
the FFT form up to 512^3; lazy inputs, the box's state, identities, argument errors."""
import ctypes

import numpy as np
import pytest

from fastbox_amd import BeamHighpass, CosmoBox, default_cosmo
from tests import corrfn_numpy as cf

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-5}          # |d xi_l| <= TOL * xi_0(0): absolute, xi crosses zero


def _box(N, L, prec, rng="device", seed=7):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng=rng, seed=seed)


def _stored(x, prec):
    """The values a plan of this precision holds for a host field."""
    return np.asarray(x, dtype=np.float64).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)


def _fields(box, cross):
    d1 = np.asarray(box.realise_density(inplace=False))
    d2 = 0.6 * d1 + np.asarray(box.realise_density(inplace=False)) if cross else None
    return d1, d2


def _compare(box, d1, d2, edges, poles, prec, brute=False, label=""):
    L = (box.Lx, box.Ly, box.Lz)
    h1 = _stored(d1, prec)
    h2 = None if d2 is None else _stored(d2, prec)
    r, xi, n = box.correlation_function(delta_x=d1, second=d2, rbins=edges, poles=poles)
    ps = (0,) if poles is None else tuple(poles)
    orr, oxi, on = cf.correlation_function(h1, h2, L, edges, poles=ps, brute=brute)
    if poles is None:
        assert xi.shape == (edges.size - 1,)
        xi = xi[None]
    else:
        assert xi.shape == (len(poles), edges.size - 1)
    for a in (r, xi, n):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.writeable
    assert np.array_equal(n, on), "npairs differ"
    m = on > 0
    assert np.array_equal(np.isnan(r), ~m) and np.all(np.isnan(xi[:, ~m]))
    assert np.all(np.abs(r[m] - orr[m]) <= 1e-14 * orr[m])             # (r = 0 exactly in a bin of s = 0 alone)
    scale = np.std(h1) * np.std(h1 if h2 is None else h2)          # xi_0(0) of the auto-correlations
    dev = np.max(np.abs(xi[:, m] - oxi[:, m])) / scale if m.any() else 0.
    print("corrfn %s N=%d %s %s nbins=%d poles=%s: max |d xi| / xi0(0) = %.3e"
          % (label, box.N, prec, "cross" if d2 is not None else "auto", edges.size - 1, ps, dev))
    assert dev <= TOL[prec]
    return r, xi, n


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("L", [1e2, (1e2, 2e2, 1e3)])
@pytest.mark.parametrize("cross", [False, True])
def test_brute_force_16(prec, L, cross):
    box = _box(16, L, prec)
    d1, d2 = _fields(box, cross)
    h = min(box.Lx, box.Ly, box.Lz) / 16
    edges = np.arange(0., 0.5 * max(box.Lx, box.Ly, box.Lz) + 0.5 * h, h)       # edges exactly on separations
    _compare(box, d1, d2, edges, [0, 2, 4], prec, brute=True, label="brute")


NB = dict(dr=2., rmin=20., rmax=200.)           # the notebooks' bins at L = 1000
CASES = [
    # N, L, prec, cross, bins, poles
    (32, 1e3, "f64", False, "default", None),
    (32, 1e3, "f32", True, "default", [0, 2, 4]),
    (64, 1e3, "f64", True, "notebook", [0, 2, 4]),
    (64, 1e3, "f32", False, "notebook", None),
    (64, (1e2, 2e2, 1e3), "f64", False, "cell", [0, 2, 4]),
    (128, 1e3, "f64", False, "cell", [0, 2, 4]),
    (128, 1e3, "f32", True, "cell", [2]),
    (128, (1e2, 2e2, 1e3), "f32", True, "default", [0, 4]),
    (256, 1e3, "f32", False, "notebook", [0, 2, 4]),
    (256, 1e3, "f64", True, "notebook", [0, 2, 4]),
    (48, 1e3, "f64", False, "default", [0, 2, 4]),
    (96, (1e2, 2e2, 1e3), "f32", True, "cell", [0, 2, 4]),
    (512, 1e3, "f32", False, "notebook", [0, 2, 4]),
]


def _edges(box, bins):
    lmin = min(box.Lx, box.Ly, box.Lz)
    if bins == "default":
        return np.arange(0., 0.5 * lmin + 0.5 * lmin / box.N, lmin / box.N)
    if bins == "notebook":
        return np.arange(NB["rmin"], NB["rmax"] + 0.5 * NB["dr"], NB["dr"])
    h = lmin / box.N                                                          # dr = the cell: edges on separations
    return np.arange(0., 0.3 * lmin + 0.5 * h, h)


@pytest.mark.parametrize("N,L,prec,cross,bins,poles", CASES)
def test_against_fft_oracle(N, L, prec, cross, bins, poles):
    box = _box(N, L, prec)
    d1, d2 = _fields(box, cross)
    _compare(box, d1, d2, _edges(box, bins), poles, prec, label=bins)


def test_default_bins_match_hostgeom():
    box = _box(32, 1e3, "f64")
    d1 = np.asarray(box.realise_density())
    r, xi, n = box.correlation_function()                                     # box.delta_x, default edges
    r2, xi2, n2 = box.correlation_function(delta_x=d1, rbins=_edges(box, "default"))
    assert np.array_equal(n, n2) and np.array_equal(xi, xi2, equal_nan=True) and np.array_equal(r, r2, equal_nan=True)
    r3, xi3, n3 = box.correlation_function(delta_x=d1, **NB)
    assert n3.size == 90


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lazy_inputs_equal_materialised(prec):
    box = _box(64, 1e3, prec)                  # (64: the size from which f32 boxes defer the redshift-space remap)
    edges = _edges(box, "notebook")
    kw = dict(rbins=edges, poles=[0, 2, 4])

    def same(lazy, label):
        a = box.correlation_function(delta_x=lazy, **kw)
        b = box.correlation_function(delta_x=np.asarray(lazy), **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), label
    dx = box.realise_density()                           # device generator: the last FFT pass still pending
    same(dx, "realise_density")
    dx2 = box.realise_density()
    same(box.lognormal(dx2), "lognormal")
    box.realise_density()
    box.realise_velocity()
    vz = box.to_real(box.velocity_k[2])
    same(box.redshift_space_density(delta_x=box.delta_x, velocity_z=vz, sigma_nl=0.), "redshift_space_density")
    filt = BeamHighpass(kpar0=0.05, kperp0=0.3)
    same(box.apply_transfer_fn(box.to_k(box.delta_x), filt).real, "apply_transfer_fn")
    # a cross-correlation with a lazy second field
    dx3 = box.realise_density(inplace=False)
    a = box.correlation_function(delta_x=dx2, second=dx3, **kw)
    b = box.correlation_function(delta_x=np.asarray(dx2), second=np.asarray(dx3), **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_box_state_is_untouched():
    box = _box(32, 1e3, "f32")
    box.realise_density()
    before = box.binned_power_spectrum()
    dx, counter, cache = box.delta_x, box._realisation, dict(box._bin_cache)
    one = box.correlation_function(poles=[0, 2, 4])
    two = box.correlation_function(poles=[0, 2, 4])
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)                           # bit-reproducible
    assert box._realisation == counter and box.delta_x is dx and box._delta_k is None
    assert box._bin_cache.keys() == cache.keys()
    after = box.binned_power_spectrum()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bin_geometry_is_recomputed_after_eviction(prec):
    """The plan keeps the data-independent sums (cells, mean separation) of the last 16 edge sets: after 17 other sets the
    first one is computed again, and the whole result -- counts and mean separations included -- is what it was."""
    box = _box(32, 1e3, prec)
    d1 = box.realise_density(inplace=False)
    first = box.correlation_function(delta_x=d1, dr=40., rmax=400., poles=[0, 2])
    for q in range(17):
        box.correlation_function(delta_x=d1, dr=41. + q, rmax=400.)
    again = box.correlation_function(delta_x=d1, dr=40., rmax=400., poles=[0, 2])
    assert np.all(first[2] > 0)                                               # no empty bin: nothing is NaN
    for x, y in zip(first, again):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_identities(prec):
    box = _box(64, 1e3, prec)
    dx = box.realise_density()
    eng = box.engine
    N3 = float(box.N) ** 3
    s1, s2 = eng.sum_real(dx), eng.sum_real(dx, squared=True)
    var = s2 / N3 - (s1 / N3) ** 2
    r, xi, n = box.correlation_function(rbins=[0., 1e-9, 1e9])
    assert n[0] == 1 and n.sum() == N3 and r[0] == 0.
    tol = 1e-12 if prec == "f64" else 1e-5
    print("corrfn zero lag %s: xi(0) / var - 1 = %.3e; sum xi / (var N^3) = %.3e"
          % (prec, xi[0] / var - 1, (xi[0] + xi[1] * n[1]) / (var * N3)))
    assert abs(xi[0] / var - 1.) <= tol
    assert abs(xi[0] + xi[1] * n[1]) <= (1e-10 if prec == "f64" else 1e-4) * var * N3


def test_argument_errors_before_device_work():
    box = _box(16, 1e2, "f32")
    box.realise_density()
    pool = {k: list(v) for k, v in box.engine._pool.items()}
    with pytest.raises(ValueError):
        box.correlation_function(second=np.zeros((8, 8, 8)))
    with pytest.raises(ValueError):
        box.correlation_function(rbins=[0., 5., 3.])
    with pytest.raises(ValueError):
        box.correlation_function(poles=[1])
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool
    other = _box(16, 1e2, "f32")
    with pytest.raises(ValueError):
        box.correlation_function(second=other.realise_density())


def test_c_entries_refuse_bad_arguments():
    from fastbox_amd import _lib
    lib = _lib.load()
    box = _box(16, 1e2, "f64")
    eng = box.engine
    dx = box.realise_density()
    wh, wr = eng.empty("half"), eng.empty("real")
    out = np.zeros(64)
    o = out.ctypes.data_as(_lib.P_double)

    def e(*v):
        a = np.array(v, dtype=np.float64)
        return a, a.ctypes.data_as(_lib.P_double)
    good, gp = e(0., 5., 10.)
    assert lib.fb_bin_separation(eng._plan, dx.ptr, gp, 2, 0, o, eng.stream) == 0
    assert out[0] + out[1] > 0
    for arr, nb, lmax in [(e(0., 5., 5.), 2, 0), (e(0., 5., 3.), 2, 0), (e(-1., 5., 10.), 2, 0), (e(0., 5., 10.), 0, 0),
                          (e(0., 5., 10.), 2, 1), (e(0., 5., 10.), 2, 6)]:
        assert lib.fb_bin_separation(eng._plan, dx.ptr, arr[1], nb, lmax, o, eng.stream) == -1
        assert lib.fb_correlation_function(eng._plan, dx.ptr, None, wh.ptr, None, wr.ptr, arr[1], nb, lmax, o, eng.stream) == -1
    assert lib.fb_correlation_function(eng._plan, dx.ptr, dx.ptr, wh.ptr, None, wr.ptr, gp, 2, 0, o, eng.stream) == -1
    assert lib.fb_cross_power_half(eng._plan, wh.ptr, None, None, 1.0, eng.stream) == -1
    assert lib.fb_cross_power_half(eng._plan, None, None, wh.ptr, 1.0, eng.stream) == -1


def test_cross_power_half_building_block():
    """fb_cross_power_half + fb_fft_c2r + fb_bin_separation, composed by hand, give what fb_correlation_function gives."""
    from fastbox_amd import _lib
    box = _box(32, 1e3, "f64")
    eng = box.engine
    d1 = box.realise_density(inplace=False)
    d2 = box.realise_density(inplace=False)
    edges = np.arange(0., 200., 10.)
    one = eng.correlation(d1, d2, edges, 4)
    h1, h2 = eng.fft_r2c(d1), eng.fft_r2c(d2)
    _lib.call("fb_cross_power_half", eng._plan, h1.ptr, h2.ptr, h2.ptr, 1.0 / 32. ** 6, eng.stream)
    xi = eng.fft_c2r(h2, scale=1.0, destroy=True)
    out = np.zeros(one.size)
    _lib.call("fb_bin_separation", eng._plan, xi.ptr, edges.ctypes.data_as(_lib.P_double), edges.size - 1, 4,
              out.ctypes.data_as(_lib.P_double), eng.stream)
    assert np.array_equal(out, one)
    # the host field xi against the FFT form itself
    oxi = cf.xi_fft(np.asarray(d1), np.asarray(d2))
    assert np.max(np.abs(np.asarray(xi) - oxi)) <= 1e-12 * np.std(np.asarray(d1)) * np.std(np.asarray(d2))


def test_more_bins_than_the_power_spectrum_binning():
    """1024 separation bins (the default edges of a 2048^3 box) with three multipoles: 106 KiB of per-wave LDS rows."""
    box = _box(256, 1e3, "f64")
    d1, _ = _fields(box, False)
    _compare(box, d1, None, np.linspace(0., 300., 1025), [0, 2, 4], "f64", label="1024 bins")


def test_default_bins_at_1024():
    """A plain call on a 1024^3 box: 512 default bins.  npairs against a host count over the folded octant, xi of the
    first 200 bins against the same cells binned through a call with those edges only."""
    N, L = 1024, 1e3
    box = _box(N, L, "f32")
    box.realise_density()
    r, xi, n = box.correlation_function(poles=[0, 2, 4])
    edges = np.arange(0., 0.5 * L + 0.5 * L / N, L / N)
    assert xi.shape == (3, 512) and n.size == 512
    h = L / N
    t = np.arange(N // 2 + 1)
    s = t * h
    mult = np.where((t == 0) | (t == N // 2), 1., 2.)
    szz = s * s
    host = np.zeros(512)
    for a in range(N // 2 + 1):
        sxy = s[a] * s[a] + s * s                                           # (s_x s_x + s_y s_y) per |m_y|
        S = np.sqrt(sxy[:, None] + szz[None, :])
        b = np.digitize(S, edges) - 1
        ok = (b >= 0) & (b < 512)
        host += np.bincount(b[ok], weights=(mult[a] * mult[:, None] * mult[None, :] * np.ones_like(S))[ok], minlength=512)
    assert np.array_equal(n, host)
    r2, xi2, n2 = box.correlation_function(rbins=edges[:201], poles=[0, 2, 4])
    assert np.array_equal(n[:200], n2)
    assert np.all(np.abs(r[1:200] - r2[1:]) <= 1e-14 * r2[1:]) and r[0] == r2[0] == 0.
    dev = np.max(np.abs(xi[:, :200] - xi2)) / xi[0, 0]
    print("corrfn default bins N=1024 f32: 512 bins; first 200 against a 200-bin call: max |d xi| / xi0(0) = %.3e" % dev)
    assert dev <= 1e-12
