"""GPU: CosmoBox.bispectrum and its C entry (fb_bispectrum) against the numpy statement of the definition (tests/bk_numpy.py)
computed on the values the plan holds; plane-wave triangles with a closed form, consistency with power_spectrum, scaling,
repeatability, lazy inputs, the box's state and argument errors.

Tolerance.  Per triple dev_t = |B_dev - B_ref| / A_t, A_t = (V^2 / N^12) sum_x |I_b1 I_b2 I_b3| / ntri_t the scale of B_t's
rounding error.  delta_ref is what the statement itself cannot resolve: for f64 its own max dev_t when the field is given with
x and y (and Lx, Ly) exchanged, which leaves B unchanged; for f32 the max dev_t between the statement with single-precision
transforms and the fp64 one.  The bound is 10 delta_ref, with the largest delta_ref over the parity cases of that precision as
the floor (an accidentally tiny delta_ref of one case does not bite)."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, hostgeom
from tests import bk_numpy as bk
from tests.test_power_spectrum_gpu import TOL as POWER_TOL

pytestmark = pytest.mark.gpu

CUBOID = (100., 130., 170.)


def _box(N, L, prec, seed=7):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng="device", seed=seed)


def _stored(x, prec):
    """The values a plan of this precision holds for a host field."""
    return np.asarray(x, dtype=np.float64).astype(np.float32 if prec == "f32" else np.float64).astype(np.float64)


def _L(box):
    return (box.Lx, box.Ly, box.Lz)


def _edges(N, L, kind):
    """The edge sets of the parity cases; L the box sides as the box reports them."""
    kf, knyq_lo, knyq_hi = 2. * np.pi / min(L), np.pi * N / max(L), np.pi * N / min(L)
    if kind == "default":
        return hostgeom.bispectrum_edges(L, N)
    if kind == "lin8":                         # 8 linear shells to (2/3) k_Nyq
        return np.linspace(0., (2. / 3.) * knyq_lo, 9)
    if kind == "nyq8":                         # 8 shells to just past k_Nyq: triangles that close through an alias
        return np.linspace(0., 1.0001 * knyq_hi, 9)
    if kind == "lattice":                      # edges exactly on the |k| of axis-aligned modes
        return np.arange(0., (2. / 3.) * knyq_lo + 0.5 * kf, kf)
    if kind == "log17":                        # 17 log-spaced shells: two tiles, the second almost empty
        return np.geomspace(3. * kf, (2. / 3.) * knyq_hi, 18)
    if kind == "one":                          # a single shell
        return np.array([2.5 * kf, 5.5 * kf])
    if kind == "lin5":
        return np.linspace(0., (2. / 3.) * knyq_lo, 6)
    if kind == "lin17":
        return np.linspace(0., 1.0001 * knyq_hi, 18)
    if kind == "lin32":                        # the most shells there are
        return np.linspace(0., 1.0001 * knyq_hi, 33)
    raise KeyError(kind)


# N, L, prec, edges.  Tiles of the contraction: nb <= 16 one, nb > 16 two; N = 2 mod 4 (18) takes the edge instances (N^3 is
# no multiple of the staging run); 18 and 24 are the generic-grid transforms; the unit-spectrum pass of every f32 case runs
# the fp64 instance of the same shape.
CASES = [
    (16, 100., "f64", "default"), (16, 100., "f32", "nyq8"), (16, CUBOID, "f32", "one"),
    (18, CUBOID, "f64", "lin8"), (18, 100., "f32", "lin8"), (18, 100., "f32", "lin17"), (18, CUBOID, "f64", "lin17"),
    (24, CUBOID, "f32", "default"), (24, CUBOID, "f64", "lattice"), (24, 100., "f64", "nyq8"),
    (32, 100., "f64", "log17"), (32, 100., "f32", "lin32"), (32, CUBOID, "f64", "lin32"), (32, 100., "f64", "one"),
    (32, 100., "f32", "lin5"), (32, 100., "f64", "lin8"),
    (64, 100., "f64", "default"), (64, 100., "f32", "lattice"), (64, CUBOID, "f32", "log17"), (64, 100., "f32", "nyq8"),
    (128, 100., "f32", "lin5"),
]
FLOOR_MAX_N = 32          # the floor of the bound is taken over the parity cases up to this size (their statements are cheap)


@functools.lru_cache(maxsize=None)
def _case(N, L, prec, kind):
    """(box, host field as stored, edges, the fp64 statement, delta_ref) of a parity case, computed once."""
    box = _box(N, L, prec)
    d = _stored(np.asarray(box.realise_density(inplace=False)), prec)
    d.setflags(write=False)
    Lb = _L(box)
    edges = _edges(N, Lb, kind)
    ref = bk.bispectrum(d, Lb, edges)
    ok = ref["ntri"] > 0
    if prec == "f64":
        other = bk.bispectrum(np.ascontiguousarray(d.transpose(1, 0, 2)), (Lb[1], Lb[0], Lb[2]), edges, ntri=ref["ntri"])
    else:
        other = bk.bispectrum(d, Lb, edges, single=True, ntri=ref["ntri"])
    dref = float(np.max(np.abs(other["B"][ok] - ref["B"][ok]) / ref["A"][ok]))
    return box, d, edges, ref, dref


@functools.lru_cache(maxsize=None)
def _floor(prec):
    return max(_case(*c)[4] for c in CASES if c[2] == prec and c[0] <= FLOOR_MAX_N)


def _bound(prec, dref=0.):
    return 10. * max(_floor(prec), dref)


@pytest.mark.parametrize("N,L,prec,kind", CASES)
def test_against_numpy(N, L, prec, kind):
    box, d, edges, ref, dref = _case(N, L, prec, kind)
    nb = edges.size - 1
    T = nb * (nb + 1) * (nb + 2) // 6
    k, B, Q, ntri = box.bispectrum(delta_x=d, kbins=edges, reduced=True)
    assert k.shape == (T, 3) and B.shape == Q.shape == ntri.shape == (T,)
    for a in (k, B, Q, ntri):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.writeable
    ok = ref["ntri"] > 0
    frac = np.count_nonzero(ok) / float(T)
    assert frac >= 0.3, "only %.0f %% of the triples have a triangle" % (100. * frac)
    assert np.array_equal(ntri, ref["ntri"]), "ntri differs in %d triples" % np.count_nonzero(ntri != ref["ntri"])
    raw = box.engine.bispectrum(box._as_real(d), edges)
    assert np.array_equal(raw[T:T + nb], ref["nmodes"]), "modes per shell differ"
    again = hostgeom.finish_bispectrum(raw, ntri, nb, _L(box), N)
    for x, y in zip((k, B, Q, ntri), again):
        assert np.array_equal(x, y, equal_nan=True), "two calls differ"
    assert np.array_equal(np.isnan(B), ~ok) and np.array_equal(np.isnan(Q), ~ok)
    assert np.array_equal(np.isnan(k), np.isnan(ref["k"]))
    krel = np.max(np.abs(k[ok] - ref["k"][ok]) / ref["k"][ok])
    bound = _bound(prec, dref)
    dev = np.max(np.abs(B[ok] - ref["B"][ok]) / ref["A"][ok])
    den = ref["B"][ok] / ref["Q"][ok]                                  # P1 P2 + P2 P3 + P3 P1
    devq = np.max(np.abs(Q[ok] - ref["Q"][ok]) * den / ref["A"][ok])
    print("bispectrum N=%d %s %s nb=%d: %d of %d triples, ntri <= %.3g equal; max |dk|/k = %.2e; max dev_t B %.3e, Q %.3e; "
          "delta_ref %.3e, bound %.3e" % (N, prec, kind, nb, np.count_nonzero(ok), T, ntri.max(), krel, dev, devq, dref, bound))
    assert krel <= 1e-14, "k: %.3e" % krel
    assert dev <= bound, "B: max dev_t %.3e > %.3e" % (dev, bound)
    assert devq <= bound, "Q: max dev_t %.3e > %.3e" % (devq, bound)      # (Q's deviation times its denominator: in B's units)


def _plane_waves(N, modes):
    x = np.indices((N, N, N)).astype(np.float64)
    return sum(np.cos(2. * np.pi * (m[0] * x[0] + m[1] * x[1] + m[2] * x[2]) / N) for m in modes)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("modes,triple,ntri,amp", [
    ([(2, 1, 0), (-1, 3, 2), (-1, -4, -2)], (1, 3, 4), 4008., 0.25),
    ([(2, 2, 1), (-2, -1, 2), (0, -1, -3)], (2, 2, 2), 1200., 1.5),
])
def test_constructed_triangle(prec, modes, triple, ntri, amp):
    """Three plane waves that close a triangle: B = amp V^2 / ntri in their triple, zero everywhere else."""
    N, L = 16, 100.
    box = _box(N, L, prec)
    Lb = _L(box)
    kf = 2. * np.pi / Lb[0]
    edges = (np.arange(9) + 0.5) * kf
    k, B, nt = box.bispectrum(delta_x=_plane_waves(N, modes), kbins=edges)
    tri = hostgeom.bispectrum_triples(8)
    t = int(np.nonzero((tri == triple).all(axis=1))[0][0])
    V = Lb[0] * Lb[1] * Lb[2]
    want = amp * V * V / ntri
    eps = 1e-13 if prec == "f64" else 2e-6       # a few roundings of the three unit-amplitude waves in the plan's precision
    rest = np.nanmax(np.abs(np.delete(B, t)))
    print("triangle %s %s: ntri %d, B / expected - 1 = %.2e, other triples / B <= %.2e" % (triple, prec, nt[t], B[t] / want - 1., rest / want))
    assert nt[t] == ntri
    assert abs(B[t] / want - 1.) <= eps
    # a triple with fewer triangles weighs the same leakage more: ntri / ntri_t
    other = np.delete(np.abs(B) * nt / ntri, t)
    assert np.nanmax(other) <= eps * want


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_shell_power_equals_power_spectrum(prec):
    """Q = B / (3 P_b^2) on the equilateral triples: the P_b it implies is power_spectrum's on the same edges."""
    box, d, edges, ref, _ = _case(32, 100., prec, "lin8")
    k, B, Q, ntri = box.bispectrum(delta_x=d, kbins=edges, reduced=True)
    kp, power, modes = box.power_spectrum(delta_x=d, kbins=edges)
    tri = hostgeom.bispectrum_triples(edges.size - 1)
    eq = np.nonzero((tri[:, 0] == tri[:, 2]) & (ntri > 0))[0]
    assert eq.size >= 5
    b = tri[eq, 0]
    implied = np.sqrt(B[eq] / (3. * Q[eq]))
    dev = np.max(np.abs(implied - power[b])) / np.max(np.abs(power[b]))
    print("P_b implied by Q vs power_spectrum %s: max |d P| / max |P| = %.3e" % (prec, dev))
    assert dev <= POWER_TOL[prec]
    assert np.max(np.abs(k[eq, 0] - kp[b]) / kp[b]) <= 1e-14


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_scaling_and_repeat(prec):
    box, d, edges, ref, dref = _case(32, 100., prec, "lin8")
    one = box.bispectrum(delta_x=d, kbins=edges, reduced=True)
    two = box.bispectrum(delta_x=d, kbins=edges, reduced=True)
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)
    a = 1.7
    scaled = box.bispectrum(delta_x=_stored(a * d, prec), kbins=edges)
    ok = ref["ntri"] > 0
    # B(a d) = a^3 B(d): the scaled field is rounded to the plan's precision once more, which the f32 bound covers
    dev = np.max(np.abs(scaled[1][ok] / a ** 3 - one[1][ok]) / ref["A"][ok])
    print("B(a d) / a^3 - B(d) %s: max dev_t %.3e, bound %.3e" % (prec, dev, _bound(prec, dref)))
    assert dev <= _bound(prec, dref)
    assert np.array_equal(scaled[2], one[3])


def test_box_state_is_untouched():
    box = _box(32, 1e3, "f32")
    box.realise_density()
    before = box.binned_power_spectrum()
    dx, counter, cache = box.delta_x, box._realisation, dict(box._bin_cache)
    one = box.bispectrum()
    two = box.bispectrum(reduced=True)
    assert len(one) == 3 and len(two) == 4 and one[0].shape == (816, 3)
    assert np.array_equal(one[1], two[1], equal_nan=True) and np.array_equal(one[2], two[3])
    assert box._realisation == counter and box.delta_x is dx and box._delta_k is None
    assert box._bin_cache.keys() == cache.keys()
    after = box.binned_power_spectrum()
    for x, y in zip(before, after):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lazy_inputs_equal_materialised(prec):
    box = _box(32, 1e3, prec)
    kw = dict(kbins=_edges(32, _L(box), "lin5"))

    def same(lazy, label):
        a = box.bispectrum(delta_x=lazy, **kw)
        b = box.bispectrum(delta_x=np.asarray(lazy), **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), label
    same(box.realise_density(), "realise_density")        # device generator: the last FFT pass still pending
    same(box.lognormal(box.realise_density()), "lognormal")
    # a log-normal field has a bispectrum, a Gaussian one only noise: the statistic tells them apart
    g = box.realise_density(inplace=False)
    kg, bg, qg, ng = box.bispectrum(delta_x=g, reduced=True, **kw)
    kl, bl, ql, nl = box.bispectrum(delta_x=box.lognormal(g), reduced=True, **kw)
    assert np.array_equal(ng, nl) and np.nanmax(np.abs(ql)) > 0


def test_argument_errors_before_device_work():
    box = _box(16, 1e2, "f32")
    box.realise_density()
    box.bispectrum(kbins=[0.1, 0.5, 0.9])
    pool = {k: list(v) for k, v in box.engine._pool.items()}
    other = _box(16, 1e2, "f32")
    bad = [dict(delta_x=np.zeros((8, 8, 8))), dict(kbins=[0., 0.5, 0.3]), dict(kbins=[0.1, 0.1]), dict(kbins=[-0.1, 0.5]),
           dict(kbins=[0.1]), dict(kbins=np.linspace(0., 1., 34)), dict(kbins=[0.1, 0.2], dk=0.1), dict(dk=0.),
           dict(dk=1e-6), dict(kbins=np.zeros((2, 3))), dict(delta_x=other.realise_density())]
    for kw in bad:
        with pytest.raises(ValueError):
            box.bispectrum(**kw)
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool


def test_c_entry():
    import ctypes
    from fastbox_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "fb_bispectrum") and "fb_bispectrum" in _lib.SIGNATURES
    box, d, edges, ref, _ = _case(16, 100., "f64", "default")
    eng = box.engine
    nb = edges.size - 1
    T = nb * (nb + 1) * (nb + 2) // 6
    real = box._as_real(d)
    wh = eng.empty("half")
    shells = eng._alloc_bytes(4 * eng.nbytes["half"])
    cubes = eng._alloc_bytes(nb * eng.nbytes["real"])
    ep = edges.ctypes.data_as(_lib.P_double)
    rec = {}
    for nwork in (1, 3, 4):                                # shells per read of the spectrum: the record does not depend on it
        out = np.zeros(T + 3 * nb)
        assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, shells.ptr, nwork, cubes.ptr, ep, nb, 0,
                                 out.ctypes.data_as(_lib.P_double), eng.stream) == 0
        rec[nwork] = out
    assert np.array_equal(rec[1], rec[3]) and np.array_equal(rec[1], rec[4])
    assert np.array_equal(rec[4], eng.bispectrum(real, edges))
    assert np.array_equal(rec[4][T:T + nb], ref["nmodes"])
    unit = np.zeros(T + 3 * nb)
    assert lib.fb_bispectrum(eng._plan, None, None, shells.ptr, 4, cubes.ptr, ep, nb, 1, unit.ctypes.data_as(_lib.P_double),
                             eng.stream) == 0
    assert np.array_equal(hostgeom.bispectrum_ntri(unit, nb, 16), ref["ntri"])
    assert np.array_equal(unit[T:T + nb], ref["nmodes"]) and np.array_equal(unit[T + 2 * nb:], ref["nmodes"])
    o = unit.ctypes.data_as(_lib.P_double)
    s4 = (shells.ptr, 4, cubes.ptr)
    assert lib.fb_bispectrum(eng._plan, None, wh.ptr, *s4, ep, nb, 0, o, eng.stream) == -1          # no field
    assert lib.fb_bispectrum(eng._plan, real.ptr, None, *s4, ep, nb, 0, o, eng.stream) == -1
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, None, 4, cubes.ptr, ep, nb, 0, o, eng.stream) == -1
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, shells.ptr, 4, None, ep, nb, 0, o, eng.stream) == -1
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, *s4, ep, 0, 0, o, eng.stream) == -1
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, *s4, ep, 33, 0, o, eng.stream) == -1
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, shells.ptr, 5, cubes.ptr, ep, nb, 0, o, eng.stream) == -1
    bad = np.array([0.3, 0.2, 0.5])
    assert lib.fb_bispectrum(eng._plan, real.ptr, wh.ptr, *s4, bad.ctypes.data_as(_lib.P_double), 2, 0, o, eng.stream) == -1
    assert b"ascending" in lib.fb_last_error()
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.fb_device_memory(ctypes.byref(free), ctypes.byref(total)) == 0 and 0 < free.value <= total.value


def test_example_bispectrum():
    """examples/example_bispectrum.py on a small grid: the log-normal box has a positive reduced bispectrum, the Gaussian
    box it was made from has none."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_bispectrum", os.path.join(root, "examples", "example_bispectrum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    q_gauss, q_lognormal = mod.main(32)
    assert q_lognormal > 0.5 and abs(q_gauss) < 0.25 * q_lognormal


def test_memory_check_precedes_device_work(monkeypatch):
    """The shell cubes that do not fit are refused before anything is allocated or launched."""
    box = _box(16, 1e2, "f32")
    box.realise_density()
    box.delta_x.ptr
    pool = {k: list(v) for k, v in box.engine._pool.items()}
    assert box.engine.free_bytes() > box.engine.bispectrum_bytes(16) > 16 * box.engine.nbytes["real"]
    monkeypatch.setattr(box.engine, "free_bytes", lambda: box.engine.bispectrum_bytes(16))
    with pytest.raises(MemoryError):                     # (a new edge set on an f32 box also needs the cubes in fp64)
        box.bispectrum()
    assert {k: list(v) for k, v in box.engine._pool.items()} == pool and "_f64_twin" not in box.engine.__dict__
