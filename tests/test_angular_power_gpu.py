"""GPU: CosmoBox.angular_power_spectrum and its C entries (fb_transverse_gram, fb_angular_power) against the numpy statement of
the definition (tests/cyl_numpy.py) computed on the values the plan holds, the identity that ties it to
cylindrical_power_spectrum, and a physics check on foreground and noise cubes.  Tolerances are those of
tests/test_power_spectrum_gpu.py, relative to max |C| of the call.

Tile-size branches of the Gram launcher (gram_shape in fb_cyl.hip: blocks of 16 MA channels) and the grid that reaches each:
    MA = 4 (N a multiple of 64)                      N = 64
    MA = 2 (a multiple of 32, not of 64)             N = 32
    MA = 1 (a multiple of 16, not of 32)             N = 16
    MA = 1, EDGE (no multiple of 16: masked block)   N = 24, 40
Every size runs auto (block pairs bi <= bj, mirrored) and cross (all pairs) in both precisions.  Chunks of a bin's modes hold
16 modes at these sizes, so bins with more than 16 modes are summed over several chunks and every bin whose count is no multiple
of 4 ends in a masked rank-4 update."""
import numpy as np
import pytest

from fastbox_amd import CosmoBox, ForegroundModel, NoiseModel, default_cosmo, hostgeom
from fastbox_amd import cosmology as _ccl
from tests import cyl_numpy as cn

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 1e-5}          # |d C| <= TOL * max |C| of the call


def _box(N, L, prec, rng="device", seed=7, **kw):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng=rng, seed=seed, **kw)


def _stored(x, prec):
    """The values a plan of this precision holds for a host field."""
    return np.asarray(x, dtype=np.float64).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)


def _fields(box, cross):
    d1 = np.asarray(box.realise_density(inplace=False)) + 0.5          # (a mean: it must not enter)
    d2 = 0.6 * d1 + np.asarray(box.realise_density(inplace=False)) if cross else None
    return d1, d2


def _L(box):
    return (box.Lx, box.Ly, box.Lz)


def _compare(box, d1, d2, edges, prec, label=""):
    kw = dict(delta_x=d1, second=d2)
    if edges is not None:
        kw["kperp_bins"] = edges
    k, cl, n = box.angular_power_spectrum(**kw)
    e = hostgeom.maps_edges(_L(box), box.N) if edges is None else np.asarray(edges, dtype=np.float64)
    ok_, ocl, on = cn.angular_power_spectrum(_stored(d1, prec), None if d2 is None else _stored(d2, prec), _L(box), e)
    nb, N = e.size - 1, box.N
    assert k.shape == (nb,) and cl.shape == (nb, N, N) and n.shape == (nb,)
    assert k.dtype == np.float64 and cl.dtype == np.float64 and n.dtype == np.int64
    assert k.flags.writeable and cl.flags.writeable
    assert np.array_equal(n, on), "modes differ"
    m = on > 0
    assert np.array_equal(np.isnan(k), ~m) and np.all(np.abs(k[m] - ok_[m]) <= 1e-14 * np.abs(ok_[m]))
    assert np.all(np.isnan(cl[~m])) and not np.any(np.isnan(cl[m]))
    scale = np.max(np.abs(ocl[m])) if m.any() else 1.
    dev = np.max(np.abs(cl[m] - ocl[m])) / scale if m.any() else 0.
    print("angular %s N=%d %s %s nb=%d: modes equal; max |d C| / max |C| = %.3e"
          % (label, N, prec, "cross" if d2 is not None else "auto", nb, dev))
    assert dev <= TOL[prec]
    if d2 is None:
        assert np.array_equal(cl[m], np.transpose(cl[m], (0, 2, 1))), "the auto result is not exactly symmetric"
    return k, cl, n


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N", [16, 24, 32, 40, 64])
def test_against_numpy(N, cross, prec):
    box = _box(N, 1e3, prec)
    d1, d2 = _fields(box, cross)
    k, cl, n = _compare(box, d1, d2, None, prec, label="default")
    assert n.sum() > N * N // 2 and n.max() > 16


@pytest.mark.parametrize("prec,cross", [("f64", False), ("f32", True)])
def test_cuboid_and_uneven_edges(prec, cross):
    box = _box(24, (1e3, 2e3, 5e2), prec)
    d1, d2 = _fields(box, cross)
    _compare(box, d1, d2, None, prec, label="cuboid default")
    kf = 2. * np.pi / 1e3
    _compare(box, d1, d2, np.array([0., 0.6 * kf, 2.3 * kf, 5.1 * kf, np.inf]), prec, label="cuboid inf")


def _constructed(name):
    """(L, edges, the expected modes per bin or None) on N = 16."""
    kf = 2. * np.pi / 100.
    if name == "four":            # exactly (+-1, 0), (0, +-1): |m| = 1; the next shell is sqrt(2)
        return 100., np.array([0.5, 1.2]) * kf, [4]
    if name == "two":             # cuboid: (0, +-1) at k = 2 pi / Ly alone; (+-1, 0) lies at twice that
        return (100., 200., 100.), np.array([0.5, 1.5]) * (2. * np.pi / 200.), [2]
    if name == "corner":          # the Nyquist corner (-8, -8) at 8 sqrt(2) = 11.31; (-8, +-7) lies at 10.63
        return 100., np.array([11., np.inf]) * kf, [1]
    if name == "residues":        # |m|^2 = 64 is (-8, 0), (0, -8) alone, the corner is one mode, every other shell a multiple of 4
        return 100., np.array([7.9, 8.05, 8.5, 11., 12.]) * kf, None
    if name == "residue3":        # the shell |m|^2 = 64 (2 modes) and the corner (1) and shells of 4 k modes between them
        return 100., np.array([7.9, np.inf]) * kf, None
    if name == "empty":           # (1.1, 1.3) kf holds no mode: between |m| = 1 and sqrt(2)
        return 100., np.array([0.9, 1.1, 1.3, 1.5]) * kf, [4, 0, 4]
    assert name == "dropped"      # modes below the first and above the last edge are dropped
    return 100., np.array([2.5, 3.5, 5.25]) * kf, None


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["four", "two", "corner", "residues", "residue3", "empty", "dropped"])
def test_constructed_edge_sets(name, prec):
    L, edges, expect = _constructed(name)
    box = _box(16, L, prec)
    for cross in (False, True):
        d1, d2 = _fields(box, cross)
        k, cl, n = _compare(box, d1, d2, edges, prec, label=name)
        if expect is not None:
            assert list(n) == expect
    if name == "residues":
        assert n[0] % 4 == 2 and n[1] % 4 == 0 and n[2] % 4 == 0 and n[3] == 1 and n[1] > 16
    if name == "residue3":
        assert n[0] % 4 == 3 and n[0] > 16
    if name == "empty":
        assert np.all(np.isnan(cl[1])) and np.isnan(k[1]) and n[1] == 0
    if name == "dropped":
        assert 0 < n.sum() < 16 * 16 - 1 - 8


def test_counts_cover_every_residue():
    """The constructed sets hold bins with counts 0, 1, 2 and 3 modulo 4 between them."""
    seen = set()
    for name in ("four", "corner", "residues", "residue3"):
        L, edges, _ = _constructed(name)
        seen |= {int(c) % 4 for c in cn.angular_power_spectrum(np.zeros((16, 16, 16)), None, (L, L, L), edges)[2] if c}
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [16, 64])
def test_identity_with_cylindrical_power(N, prec):
    """P(b, m) = (Lz / N^2) sum_{nu, nu'} C_b(nu, nu') cos(2 pi m (nu - nu') / N) for the same k_perp edges with edges[0] > 0
    and the default one-bin-per-|m_z| k_par edges; modes(b, m) = modes_b (1 if m in {0, N/2} else 2)."""
    box = _box(N, (1e3, 1e3, 2e3), prec)
    d = box.realise_density(inplace=False)
    edges = hostgeom.maps_edges(_L(box), N)
    assert edges[0] > 0
    kperp, kpar, power, modes = box.cylindrical_power_spectrum(delta_x=d, kperp_bins=edges)
    k, cl, mb = box.angular_power_spectrum(delta_x=d, kperp_bins=edges)
    mult = np.where((np.arange(N // 2 + 1) == 0) | (np.arange(N // 2 + 1) == N // 2), 1, 2)
    assert np.array_equal(modes, mb[:, None] * mult[None, :])
    m = mb > 0
    rhs = cn.power_from_maps(cl[m], box.Lz)
    dev = np.max(np.abs(rhs - power[m])) / np.max(np.abs(power[m]))
    print("identity N=%d %s: max |P - (Lz / N^2) sum C cos| / max |P| = %.3e" % (N, prec, dev))
    assert dev <= TOL[prec]


def test_collapse_and_angular_options():
    box = _box(24, 1e3, "f64", redshift=0.8)
    d1, d2 = _fields(box, True)
    k, cl, n = box.angular_power_spectrum(delta_x=d1, second=d2)
    kc, clc, nc = box.angular_power_spectrum(delta_x=d1, second=d2, collapse=True)
    assert clc.shape == (k.size, 24) and np.array_equal(kc, k, equal_nan=True) and np.array_equal(nc, n)
    want = cn.collapse(cl)
    m = n > 0
    assert np.all(np.abs(clc[m] - want[m]) <= 1e-13 * np.max(np.abs(want[m])))
    for z, zz in ((None, 0.8), (1.5, 1.5)):
        r = _ccl.comoving_angular_distance(box.cosmo, 1. / (1. + zz))
        ell, cla, na = box.angular_power_spectrum(delta_x=d1, second=d2, angular=True, redshift=z)
        assert np.array_equal(na, n) and np.array_equal(ell, k * r, equal_nan=True)
        assert np.array_equal(cla, cl / r ** 2, equal_nan=True)
    ell, clb, nb_ = box.angular_power_spectrum(delta_x=d1, second=d2, angular=True, collapse=True)
    r = _ccl.comoving_angular_distance(box.cosmo, 1. / 1.8)
    assert np.array_equal(clb, clc / r ** 2, equal_nan=True)


def test_memory_error_before_any_kernel(monkeypatch):
    box = _box(16, 1e2, "f32")
    d = box.realise_density(inplace=False)
    eng = box.engine
    nb = hostgeom.maps_edges(_L(box), 16).size - 1
    need = eng.angular_power_bytes(nb, False)
    assert need >= eng.nbytes["full"] + (nb + 1) * 16 * 16 * 8 + nb * 16 * 16 * 8     # cube, partials, result
    assert eng.angular_power_bytes(nb, True) >= need + eng.nbytes["full"]
    calls = []
    monkeypatch.setattr(eng, "angular_power", lambda *a, **k: calls.append(a))
    monkeypatch.setattr(eng, "free_bytes", lambda: need - 1)
    with pytest.raises(MemoryError):
        box.angular_power_spectrum(delta_x=d)
    assert not calls
    monkeypatch.undo()
    assert box.angular_power_spectrum(delta_x=d)[1].shape[1:] == (16, 16)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_repeatability_lazy_inputs_and_state(prec):
    box = _box(32, 1e3, prec)
    other = box.realise_density(inplace=False)
    box.realise_density()
    before = box.binned_power_spectrum()
    dx, counter, cache = box.delta_x, box._realisation, dict(box._bin_cache)
    one = box.angular_power_spectrum()
    two = box.angular_power_spectrum()
    host = box.angular_power_spectrum(delta_x=np.asarray(dx))
    for x, y, z in zip(one, two, host):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)
    a = box.angular_power_spectrum(second=other)
    b = box.angular_power_spectrum(second=np.asarray(other))
    c = box.angular_power_spectrum(delta_x=other, second=dx)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    # the first index belongs to delta_x, the second to `second`
    m = a[2] > 0
    assert np.max(np.abs(a[1][m] - np.transpose(c[1][m], (0, 2, 1)))) <= TOL[prec] * np.max(np.abs(a[1][m]))
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
           dict(kperp_bins=[-0.1, 0.5]), dict(kperp_bins=[0.3]), dict(dk_perp=0.), dict(kperp_bins=np.linspace(0., 10., 258)),
           dict(angular=True, redshift=-2.), dict(angular=True, redshift=np.nan)]
    for kw in bad:
        with pytest.raises(ValueError):
            box.angular_power_spectrum(**kw)
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool
    other = _box(16, 1e2, "f32")
    with pytest.raises(ValueError):
        box.angular_power_spectrum(second=other.realise_density())


def test_c_entries():
    from fastbox_amd import _lib
    lib = _lib.load()
    box = _box(24, (1e3, 2e3, 5e2), "f64")
    eng = box.engine
    N = 24
    d1 = box.realise_density(inplace=False)
    d2 = box.realise_density(inplace=False)
    edges = np.array([0.004, 0.01, 0.02, 0.05, np.inf])
    nb = edges.size - 1
    ep = edges.ctypes.data_as(_lib.P_double)
    wb = lib.fb_transverse_gram_work_bytes(eng._plan, nb, 1)
    assert wb >= (nb + 1) * N * N * 8 and lib.fb_transverse_gram_work_bytes(eng._plan, nb, 0) >= (nb + 1) * N * N * 8
    work, cl_dev = eng._alloc_bytes(wb), eng._alloc_bytes(nb * N * N * 8)
    f1, f2 = eng.empty("full"), eng.empty("full")
    rec = np.zeros(2 * nb)
    rp = rec.ctypes.data_as(_lib.P_double)

    def fetch():
        out = np.empty((nb, N, N))
        _lib.call("fb_memcpy_d2h", out.ctypes.data_as(_lib.ctypes.c_void_p), cl_dev.ptr, out.nbytes, eng.stream)
        return out
    assert lib.fb_angular_power(eng._plan, d1.ptr, d2.ptr, f1.ptr, f2.ptr, ep, nb, cl_dev.ptr, work.ptr, rp, eng.stream) == 0
    one, rec1 = fetch(), rec.copy()
    # the Gram entry on cubes transformed separately gives the same result
    for d, f in ((d1, f1), (d2, f2)):
        _lib.call("fb_real_to_complex", eng._plan, d.ptr, f.ptr, eng.stream)
        _lib.call("fb_fft_transverse", eng._plan, f.ptr, -1, eng.stream)
    _lib.call("fb_transverse_gram", eng._plan, f1.ptr, f2.ptr, ep, nb, cl_dev.ptr, work.ptr, rp, eng.stream)
    assert np.array_equal(one, fetch()) and np.array_equal(rec, rec1)
    k, cl, n = cn.angular_power_spectrum(np.asarray(d1), np.asarray(d2), _L(box), edges)
    assert np.array_equal(rec[:nb], n) and np.all(np.abs(rec[nb:] - k * n) <= 1e-14 * k * n)
    assert np.max(np.abs(one - cl)) <= 1e-11 * np.max(np.abs(cl))
    # invalid arguments
    def e(*v):
        a = np.array(v, dtype=np.float64)
        return a, a.ctypes.data_as(_lib.P_double)
    good = e(0.01, 0.05, 0.1)
    for arr, n_ in [(e(0., 0.05, 0.05), 2), (e(-1., 0.05, 0.1), 2), (e(0., np.nan, 0.1), 2), (good, 0), (good, 257)]:
        assert lib.fb_transverse_gram(eng._plan, f1.ptr, None, arr[1], n_, cl_dev.ptr, work.ptr, rp, eng.stream) == -1
        assert lib.fb_angular_power(eng._plan, d1.ptr, None, f1.ptr, None, arr[1], n_, cl_dev.ptr, work.ptr, rp, eng.stream) == -1
    assert lib.fb_angular_power(eng._plan, d1.ptr, d2.ptr, f1.ptr, None, good[1], 2, cl_dev.ptr, work.ptr, rp, eng.stream) == -1
    assert lib.fb_transverse_gram(eng._plan, None, None, good[1], 2, cl_dev.ptr, work.ptr, rp, eng.stream) == -1
    assert lib.fb_transverse_gram(eng._plan, f1.ptr, None, good[1], 2, None, work.ptr, rp, eng.stream) == -1
    assert lib.fb_transverse_gram(eng._plan, f1.ptr, None, good[1], 2, cl_dev.ptr, None, rp, eng.stream) == -1


def _coefficients(cl):
    dg = np.sqrt(np.einsum("bii->bi", cl))
    return cl / (dg[:, :, None] * dg[:, None, :])


def test_foregrounds_are_coherent_and_noise_is_not():
    """The channel correlation coefficient C_b(nu, nu') / sqrt(C_b(nu, nu) C_b(nu', nu')): above 0.99 everywhere for a foreground
    cube (a power law in frequency along every line of sight); for radiometer noise (independent channels) the off-diagonal
    coefficients scatter with 1 / sqrt(modes_b), bounded here at 5 / sqrt(modes_b) in the bins with at least 100 modes
    (tests/test_cylindrical_cpu.py checks that bound on numpy white noise of this shape).  The foreground amplitude map is
    not smoothed: a smoothed map leaves the high-k_perp bins nothing but the rounding of the transform, whose coefficient
    means nothing."""
    N = 64
    box = _box(N, (4e3, 4e3, 4e3), "f64", redshift=0.8)
    fg = ForegroundModel(box)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., redshift=box.redshift)
    alpha = fg.realise_spectral_index(mean_spec_idx=2.07, std_spec_idx=0.0002, smoothing_scale=15., redshift=box.redshift)
    cube = fg.construct_cube(fg_map, alpha, freq_ref=130., redshift=box.redshift)
    k, cl, n = box.angular_power_spectrum(delta_x=cube)
    m = n > 0
    r = _coefficients(cl[m])
    print("foreground cube: min channel correlation coefficient %.6f over %d bins" % (r.min(), m.sum()))
    assert m.sum() >= 30 and r.min() > 0.99
    noise = NoiseModel(box).realise_radiometer_noise(Tinst=18., tp=2., fov=1., Ndish=64)
    k, cl, n = box.angular_power_spectrum(delta_x=noise)
    sel = n >= 100
    assert sel.sum() >= 10
    off = ~np.eye(N, dtype=bool)
    r = _coefficients(cl[sel])
    worst = np.max(np.abs(r[:, off]) * np.sqrt(n[sel])[:, None])
    print("noise cube: max |coefficient| sqrt(modes) = %.3f over %d bins (bound 5)" % (worst, sel.sum()))
    assert worst <= 5.
    assert np.all(np.abs(np.mean(r[:, off], axis=1)) <= 5. / np.sqrt(n[sel]) / np.sqrt(N))
