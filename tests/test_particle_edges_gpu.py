"""GPU: the halo, painting and COLA kernels (fb_halo.hip, fb_cola.hip) on the constructed cases of tests/particle_cases.py, in
both precisions: the Poisson draw over the whole range of expected counts against scipy's exact CDF, every path of the
catalogue's tables, painting on nodes, midpoints and the seam against meshes written down from the window definitions, and the
COLA entry points one stage at a time.  What each case is for, and the property that keeps it from being vacuous, is asserted
on the CPU by tests/test_particle_cases_cpu.py.  Every test is at N <= 64."""
import ctypes
import functools
import math

import numpy as np
import pytest

from fastbox_amd import CosmoBox, _lib, cola, default_cosmo, rng
from fastbox_amd.device import REAL
from fastbox_amd.halos import HaloDistribution
from tests import cola_numpy as cn
from tests import halos_numpy as hn
from tests import particle_cases as pc
from tests.test_fft_gpu import TOL

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}


@functools.lru_cache(maxsize=None)
def _box(N, L, prec, seed=7):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng="device", seed=seed)


def _hd(box):
    return HaloDistribution(box, (1e12, 1e15), 10)


def _stored(x, prec):
    return cn.stored(x, DT[prec])


# ---- 1. Poisson counts over the whole range ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_poisson_counts_bracket_their_uniforms(prec):
    """Every count k brackets its uniform in scipy's CDF: cdf(k - 1) - s <= u < cdf(k) + s, s = 8 units of
    2^-52 max(floor(lam) ln lam, 1) (particle_cases.poisson_unit).  Measured on an MI355X: see DESIGN.md, halo tracers."""
    N, real = 32, 3
    b = pc.poisson_box(N)
    box = _box(N, b["L"], prec)
    hd = _hd(box)
    lam = hd.expected_counts(b["delta"], b["nbar"], b["bias"])
    np.testing.assert_array_equal(lam, hn.expected_counts(b["delta"], b["nbar"], b["bias"], b["L"]))
    assert lam[b["top"]] == pc.LAM_MAX == lam.max()
    row = lam[b["int_row"]]
    assert np.array_equal(row, np.floor(row)) and row.max() > 1.5e7
    k = np.asarray(hd.halo_count_field(b["delta"], b["nbar"], b["bias"], realisation=real))
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0.
    u = rng.poisson_uniforms(N ** 3, box.seed, real)
    slack, nppf = pc.poisson_bracket(k, lam, u)
    print("%s: the device needs %.3f units; %d of %d voxels differ from poisson.ppf; lam = 2^24 draws 2^24 %+d"
          % (prec, slack, nppf, N ** 3, k[b["top"]] - pc.LAM_MAX))
    assert slack <= 8., "slack %.3f units, %d voxels differ from ppf" % (slack, nppf)
    assert abs(k[b["top"]] - pc.LAM_MAX) < 8 * 4096.                  # 2^24 is drawn: within 8 sigma of it


@pytest.mark.parametrize("prec", PRECS)
def test_overflow_flag_from_any_lane(prec):
    """lam = 2^24 (1 + 2^-20) exactly, or +inf, in one voxel raises; 2^24 in the same voxel draws."""
    N = 32
    b = pc.poisson_box(N)
    hd = _hd(_box(N, b["L"], prec))
    for name, vox, nbar, delta in pc.overflow_boxes(N):
        lam = hd.expected_counts(delta, nbar, 1.)
        assert lam[vox] == (pc.LAM_MAX + 16. if name.startswith("above") else np.inf) and np.sum(lam > pc.LAM_MAX) == 1, name
        with pytest.raises(ValueError, match="2\\^24"):
            hd.halo_count_field(delta, nbar, 1., realisation=1)
        at_limit = nbar.copy()
        at_limit[vox] = pc.LAM_MAX
        assert hd.expected_counts(delta, at_limit, 1.)[vox] == pc.LAM_MAX
        k = np.asarray(hd.halo_count_field(delta, at_limit, 1., realisation=1))     # the flag is cleared: the limit draws
        assert abs(k[vox] - pc.LAM_MAX) < 8 * 4096.


def test_a_draw_above_the_limit_is_rounded_on_f32_plans():
    """The limit bounds lam, not the draw (sigma = 4096 at 2^24).  At particle_cases.ODD_DRAW the lam = 2^24 voxel draws 2^24 + 811:
    the f64 plan holds it, the f32 plan holds the nearest fp32, 2^24 + 812; every other count is the same on both plans."""
    N = 32
    b = pc.poisson_box(N)
    seed, real = pc.ODD_DRAW
    k = {}
    for prec in PRECS:
        box = _box(N, b["L"], prec, seed)
        k[prec] = np.asarray(_hd(box).halo_count_field(b["delta"], b["nbar"], b["bias"], realisation=real))
    assert k["f64"][b["top"]] == 2 ** 24 + 811 and k["f32"][b["top"]] == 2 ** 24 + 812
    np.testing.assert_array_equal(k["f32"], k["f64"].astype(np.float32).astype(np.float64))
    assert np.sum(k["f32"] != k["f64"]) == np.sum((k["f64"] > 2 ** 24) & (k["f64"] % 2 == 1)) >= 1


@pytest.mark.parametrize("prec", PRECS)
def test_lognormal_extremes(prec):
    """bias delta in [-30, 30]: the f32 plan subtracts the maximum before the exponential, the f64 plan does not.  The bound is
    the fp64 statement's own sensitivity to that shift, times 10, and at least 1e-13."""
    N = 32
    L = (float(N),) * 3
    delta, bias = pc.lognormal_box(N)
    ref, shifted = pc.lognormal_statements(delta, bias, L)
    bound = max(10. * pc.lognormal_deviation(shifted, ref, 1.), 1e-13)
    got = _hd(_box(N, L, prec)).expected_counts(delta, 1., bias, lognormal=True)
    err = pc.lognormal_deviation(got, ref, 1.)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("prec", PRECS)
def test_parameter_fields_are_indexed_per_voxel(prec):
    N, L = 32, (64., 64., 64.)
    box = _box(N, L, prec)
    hd = _hd(box)
    delta, nbar, bias = [np.ascontiguousarray(np.broadcast_to(a, (N, N, N))) for a in pc.field_params(N)]
    want = hn.expected_counts(delta, nbar, bias, L)
    dev = lambda a: box.engine.upload(a, REAL)                         # noqa: E731  (the plan's precision)
    counts = []
    for nb, bs in ((nbar, bias), (dev(nbar), bias), (nbar, dev(bias)), (dev(nbar), dev(bias))):
        np.testing.assert_array_equal(hd.expected_counts(delta, nb, bs), want)
        counts.append(np.asarray(hd.halo_count_field(delta, nb, bs, realisation=2)))
    for c in counts[1:]:
        np.testing.assert_array_equal(c, counts[0])
    ref = rng.stream_poisson(want, box.seed, 2)
    assert np.mean(counts[0] != ref) <= 1e-4 and np.max(np.abs(counts[0] - ref)) <= 1


# ---- 2. catalogue tables ------------------------------------------------------------------------------------------------------
CAT_L = (640., 650., 660.)


@functools.lru_cache(maxsize=None)
def _catalogue_reference(name):
    c = pc.catalogue_counts(name)
    ref = hn.catalogue(c, CAT_L)
    ref.setflags(write=False)
    return c, ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["atomic", "carry", "doubling"])
def test_catalogue_table_paths(prec, name):
    """'atomic': counts >= 4096 go through global atomics, in several tiles and twice within one step of a tile.  'carry':
    313 chunks, two turns of the top-level scan.  'doubling': (kmax + 1) 64 > 2^25, so cat_emit doubles the tile to 8192 voxels
    and 32 tiles (particle_cases.table_layout restates its loop); voxels of equal count on both sides of every old and new
    tile boundary keep the reference's order only if the tables follow."""
    N = 64
    c, ref = _catalogue_reference(name)
    box = _box(N, CAT_L, prec)
    hd = _hd(box)
    cat = hd.realise_halo_catalogue(c)
    assert len(cat) == ref.shape[0]
    np.testing.assert_array_equal(np.asarray(cat), ref)
    if name == "atomic":
        cs = hd.realise_halo_catalogue(c, scatter=True, realisation=4)
        np.testing.assert_array_equal(np.asarray(cs), hn.catalogue(c, CAT_L, rng.scatter_uniforms(len(cs), box.seed, 4)))


@pytest.mark.parametrize("prec", PRECS)
def test_bad_device_counts_are_refused(prec):
    N, L = 16, (160., 170., 180.)
    box = _box(N, L, prec)
    hd = _hd(box)
    good = np.random.RandomState(1).poisson(0.7, (N, N, N))
    for bad in (-1., 0.5, np.nan, np.inf):
        a = good.astype(np.float64)
        a[N - 1, N - 1, N - 1] = bad
        with pytest.raises(_lib.FastBoxError, match="non-negative integers"):
            hd.realise_halo_catalogue(box.engine.upload(a, REAL))
        np.testing.assert_array_equal(np.asarray(hd.realise_halo_catalogue(box.engine.upload(good, REAL))),
                                      hn.catalogue(good, L))


# ---- 3. painting --------------------------------------------------------------------------------------------------------------
GEOS = pc.paint_geometries()


def _paint(box, pos, window, w=None, comp=False):
    return np.asarray(box.paint_catalogue(np.ascontiguousarray(pos), weights=w, window=window, compensated=comp))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", GEOS)
def test_paint_known_weights(N, L, window, prec):
    box = _box(N, L, prec)
    pos, _ = pc.paint_positions(N, L)
    w = np.arange(1., pos.shape[0] + 1.)
    np.testing.assert_array_equal(_paint(box, pos, window, w), _stored(pc.expected_mesh(pos, N, L, window, w), prec))
    # one particle at a time: nothing cancels between particles
    for p in range(pos.shape[0]):
        np.testing.assert_array_equal(_paint(box, pos[p:p + 1], window), pc.expected_mesh(pos[p:p + 1], N, L, window))
    below, at0 = pc.below_zero_positions(N, L)
    got = _paint(box, below, window)
    np.testing.assert_array_equal(got, pc.expected_mesh(at0, N, L, window))
    np.testing.assert_array_equal(got, _paint(box, at0, window))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
def test_paint_totals(window, prec):
    """The total of the mesh is the total of the weights: exactly on an fp64 plan wherever the definition's mesh is exact in
    fp64 (two roundings per node, the high word's conversion and the sum of the two words, for TSC with weights of 1 beside
    2^40); on an fp32 plan to one fp32 rounding per node plus half a unit 2^-F of the fixed point per share,
    F = particle_cases.paint_exponent: 53 for the small weights, where every share is exact, 18 beside 2^40."""
    N, L = GEOS[1]
    n = 200
    box = _box(N, L, prec)
    pos = pc.dyadic_cloud(N, L, n, 21)
    shares = pc.expected_mesh(pos, N, L, window, count=True)
    for name, (w, total) in pc.weight_sets(n).items():
        want, exact = pc.expected_mesh(pos, N, L, window, w, return_exact=True)
        got = _paint(box, pos, window, w)
        if prec == "f64":
            tol = np.zeros_like(want) if exact else 2. ** -52 * np.abs(want)
        else:
            tol = 2. ** -24 * np.abs(want) + shares * 2. ** -(pc.paint_exponent(w, n) + 1) * (1 + 2. ** -23)
        assert np.all(np.abs(got - want) <= tol), name
        assert abs(math.fsum(got.reshape(-1)) - total) <= tol.sum() + (0. if exact else 2. ** -53 * np.abs(want).sum()), name


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
def test_paint_all_mass_on_one_node(window, prec):
    N, L = GEOS[0]
    box = _box(N, L, prec)
    node = (N - 1, 0, 5)
    one = pc.expected_mesh(np.array([node]) * (np.asarray(L) / N), N, L, window)
    pos = np.tile(np.array(node) * (np.asarray(L) / N), (2 ** 20, 1))
    for w, total in ((None, 2. ** 20), (np.full(2 ** 20, 2. ** 30), 2. ** 50)):
        np.testing.assert_array_equal(_paint(box, pos, window, w), one * total)       # exact in fp32 as well: 27 2^44 at most


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", GEOS)
def test_paint_translation_and_reflection(N, L, window, prec):
    """Bitwise: positions are multiples of an eighth of a cell, so the shifted and the mirrored fractions are exact.  NGP is
    mirrored without the cell midpoints: a particle on a midpoint belongs to the upper node, and so does its mirror image."""
    box = _box(N, L, prec)
    n = 300
    cell = np.asarray(L) / N
    pos = pc.dyadic_cloud(N, L, n, 33, ties=(window != "ngp"))
    w = pc.weight_sets(n, seed=6)["signed"][0]
    base = _paint(box, pos, window, w)
    np.testing.assert_array_equal(base, _stored(pc.expected_mesh(pos, N, L, window, w), prec))
    shift = np.array([3, -N - 2, 2 * N + 1])
    np.testing.assert_array_equal(_paint(box, pos + shift * cell, window, w), np.roll(base, shift, axis=(0, 1, 2)))
    np.testing.assert_array_equal(_paint(box, np.asarray(L) - pos, window, w), pc.reflect_mesh(base))
    if window == "ngp":
        tie = np.array([[4.5, 3., 3.]]) * cell
        assert _paint(box, tie, window)[5, 3, 3] == 1. and _paint(box, np.asarray(L) - tie, window)[N - 4, N - 3, N - 3] == 1.


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
def test_paint_skips_non_finite_and_empty(window, prec):
    N, L = GEOS[1]
    box = _box(N, L, prec)
    pos = pc.dyadic_cloud(N, L, 60, 44)
    w = np.arange(1., 61.)
    bad = pos.copy()
    rows = [2, 11, 30, 31, 59]
    for r, (a, v) in zip(rows, [(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (2, np.nan)]):
        bad[r, a] = v
    keep = np.setdiff1d(np.arange(60), rows)
    want = pc.expected_mesh(pos[keep], N, L, window, w[keep])
    np.testing.assert_array_equal(_paint(box, bad, window, w), want)
    np.testing.assert_array_equal(_paint(box, pos[keep], window, w[keep]), want)
    for comp in (False, True):
        assert not _paint(box, np.zeros((0, 3)), window, comp=comp).any()
    assert not _paint(box, bad[rows], window, w[rows]).any()            # nothing but skipped particles


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", GEOS)
def test_compensated_spike(N, L, window, prec):
    """A unit particle on a node, compensated: the closed-form spectrum of the painted spike over prod sinc^p, back in real
    space.  Bound: the forward transform is off by TOL (tests/test_fft_gpu.py) of its largest mode, 1, in every mode; the
    division amplifies that by at most max 1 / prod sinc^p; the inverse transform adds TOL of its largest output."""
    box = _box(N, L, prec)
    node = (N - 1, 0, 5)
    pos = np.array([node]) * (np.asarray(L) / N)
    spec = pc.compensated_spike_spectrum(node, N, window)
    want = np.fft.ifftn(spec).real
    got = _paint(box, pos, window, comp=True)
    err = np.max(np.abs(got - want))
    assert err <= TOL[prec] * (np.max(np.abs(spec)) + np.max(np.abs(want))), err
    assert np.max(np.abs(spec)) > 1.5 and np.max(np.abs(want)) > 1.                # not a unit spike any more


# ---- 4. COLA, stage by stage --------------------------------------------------------------------------------------------------
COLA_GEOS = pc.cola_geometries()
_VP = ctypes.c_void_p


class Stages(object):
    """The COLA entry points on the buffers of Engine.cola_buffers(), with host arrays in and out."""

    def __init__(self, N, L, prec):
        self.N, self.L, self.prec, self.dt = N, L, prec, DT[prec]
        self.box = _box(N, L, prec)
        self.eng = self.box.engine
        self.P, self.S = self.eng._plan, self.eng.stream
        self.st = self.eng.cola_buffers()
        self.n3 = N ** 3

    def ptr(self, name):
        return self.st[name].ptr

    def put_at(self, ptr, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        _lib.call("fb_memcpy_h2d", ptr, a.ctypes.data_as(_VP), a.nbytes, self.S)
        self.eng.sync()

    def put(self, name, a):
        """pos: (N^3, 3) fp64; count, delta: (N, N, N); the rest (3, N, N, N), in the plan's precision."""
        self.put_at(self.ptr(name), a, np.float64 if name == "pos" else self.dt)

    def get_at(self, ptr, shape, dtype):
        h = np.empty(shape, dtype=dtype)
        _lib.call("fb_memcpy_d2h", h.ctypes.data_as(_VP), ptr, h.nbytes, self.S)
        self.eng.sync()
        return h

    def get(self, name, raw=False):
        N = self.N
        if name == "pos":
            return self.get_at(self.ptr(name), (self.n3, 3), np.float64)
        h = self.get_at(self.ptr(name), (N, N, N) if name in ("count", "delta") else (3, N, N, N), self.dt)
        return h if raw else h.astype(np.float64)

    def lpt(self, delta0):
        d = self.eng.upload(delta0, REAL)
        _lib.call("fb_cola_lpt", self.P, d.ptr, self.ptr("psi1"), self.ptr("psi2"), self.ptr("force"), self.ptr("h1"),
                  self.ptr("h2"), self.S)
        self.eng.sync()

    def init(self, d1, d2, pres=True):
        _lib.call("fb_cola_init", self.P, self.ptr("psi1"), self.ptr("psi2"), float(d1), float(d2), self.ptr("pos"),
                  self.ptr("pres") if pres else None, self.S)

    def force(self, coef, with_force=True):
        f = with_force
        _lib.call("fb_cola_force", self.P, self.ptr("pos"), self.ptr("count"), self.ptr("delta"), self.ptr("force") if f else None,
                  float(coef), self.ptr("h1") if f else None, self.ptr("h2") if f else None, self.S)

    def kick(self, coef, drift):
        c = np.ascontiguousarray(coef, dtype=np.float64)
        _lib.call("fb_cola_kick", self.P, self.ptr("force"), self.ptr("psi1"), self.ptr("psi2"), self.ptr("pres"), self.ptr("pos"),
                  c.ctypes.data_as(_lib.P_double), int(drift), self.S)
        self.eng.sync()


def _dev(a, ref, scale=None):
    return float(np.max(np.abs(np.asarray(a) - ref)) / (np.max(np.abs(ref)) if scale is None else scale))


def _transform_bound(prec, ref32, ref64, scale=None):
    """Stages with transforms.  f64 plan: 1e-10 of the largest magnitude, as the parity tests.  f32 plan: 4 delta_ref, delta_ref
    the deviation of the float32 statement from the fp64 statement -- the device's transform is another algorithm of the same
    precision.  Returns (bound, delta_ref)."""
    dref = _dev(ref32, ref64, scale)
    return (1e-10 if prec == "f64" else 4. * dref), dref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_lpt_closed_forms_and_statement(N, L, prec):
    s = Stages(N, L, prec)
    report = []
    # a Nyquist wave along each axis: no displacement at all, to rounding.  The multiplier is zero on the wave's own mode, so what
    # is left is the transforms' rounding.  TOL (tests/test_fft_gpu.py) bounds a transform's error relative to its largest
    # magnitude; taken norm-wise, the forward transform of the wave (one mode of A N^3) leaves an error spectrum of 2-norm
    # TOL A N^3, the multiplier is at most 1 / k_min = L / 2 pi, and by Parseval the inverse transform (1 / N^3) turns that into
    # an rms of TOL A L / 2 pi; storing the product and the inverse transform add as much again each: rms <= 3 TOL A L / 2 pi.
    # The largest of N^3 <= 32768 such residuals, sums of many roundings, is allowed 8 times the rms bound (4.6 is the
    # expectation for Gaussian residuals).  Psi2 comes from the source, wave x residual: the same with A^2.
    for axis in range(3):
        s.lpt(pc.nyquist_wave(N, axis))
        for name, amp in (("psi1", 0.25), ("psi2", 0.25 ** 2)):
            got = s.get(name)
            unit = TOL[prec] * amp * L / (2 * np.pi)
            rms, top = np.sqrt(np.mean(got ** 2)) / unit, np.max(np.abs(got)) / unit
            msg = "nyquist axis %d %s N=%d %s: rms %.2e, max %.2e of TOL A L / 2 pi" % (axis, name, N, prec, rms, top)
            report.append(msg)
            assert rms <= 3. and top <= 24., msg
    # two waves against the closed form, one Gaussian field against the statement
    d2, w1, w2 = pc.two_waves(N, L)
    g = pc.gaussian_field(N)
    for tag, d, want in (("waves", d2, (w1, w2)), ("gauss", g, None)):
        din = _stored(d, prec)
        ref64 = cn.lpt(din, L)
        ref32 = cn.lpt(din, L, np.float32)
        s.lpt(d)
        for j, name in enumerate(("psi1", "psi2")):
            bound, dref = _transform_bound(prec, ref32[j], ref64[j])
            got = s.get(name)
            err = _dev(got, ref64[j])
            report.append("%s %s N=%d %s: delta_ref %.2e device %.2e" % (tag, name, N, prec, dref, err))
            assert err <= bound, report[-1]
            if want is not None:
                # the closed form is that of the field before it is stored: on an f32 plan the stored cosine differs from it,
                # by what the fp64 statement makes of the stored field (1e-15 on an f64 plan)
                d_in = _dev(ref64[j], want[j])
                assert prec == "f32" or d_in <= 1e-12, d_in
                assert _dev(got, want[j]) <= bound + d_in, report[-1]
                assert np.max(np.abs(got[0])) <= (bound + d_in) * np.max(np.abs(want[j]))     # the x component vanishes
    print("\n".join(report))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_init_wraps_into_the_box(N, L, prec):
    s = Stages(N, L, prec)
    psi1, psi2, want, special = pc.init_displacements(N, L)
    s.put("psi1", psi1)
    s.put("psi2", psi2)
    for with_pres in (True, False):
        s.put("pres", np.full((3, N, N, N), 7.))
        s.put("pos", np.full((N ** 3, 3), -1.))
        s.init(1., 1., pres=with_pres)
        pos = s.get("pos")
        np.testing.assert_array_equal(pos, want)
        assert np.all((pos >= 0.) & (pos < L)) and not np.any(np.signbit(pos))
        assert np.all(s.get("pres") == (0. if with_pres else 7.))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_force_count_delta_and_components(N, L, prec):
    s = Stages(N, L, prec)
    pos = pc.tiled_positions(N, L)
    s.put("pos", pos)
    s.put("force", np.full((3, N, N, N), -777.))
    s.force(1.5, with_force=False)
    count = cn.paint(pos, N, L)                                        # dyadic: exact
    np.testing.assert_array_equal(s.get("count"), _stored(count, prec))
    np.testing.assert_array_equal(s.get("delta"), _stored(_stored(count, prec) - 1., prec))
    assert np.all(s.get("force") == -777.)
    s.force(1.5)
    np.testing.assert_array_equal(s.get("count"), _stored(count, prec))
    ref64, ref32 = cn.force(pos, N, L, 1.5)[1], cn.force(pos, N, L, 1.5, np.float32)[1]
    bound, dref = _transform_bound(prec, ref32, ref64)
    err = _dev(s.get("force"), ref64)
    msg = "force N=%d %s: delta_ref %.2e device %.2e" % (N, prec, dref, err)
    print(msg)
    assert err <= bound, msg


def _kick_bounds(F, p1, p2, pres, pos, N, L, coef, dtype):
    """Transform-free stages: the device and the statement evaluate the same expression, so they may differ by the order and the
    intermediate roundings of its fp64 sums, particle_cases.sum_bound over the magnitudes of the terms, and by one rounding of
    each stored value, particle_cases.storage_bound.  The read-out's terms are the eight w |F|; the kick adds p_res, dP1 Psi1
    and dP2 Psi2; the position carries the bound of p_res through Dr and adds its own terms, the box length among them (the
    wrap subtracts a multiple of it)."""
    cK, dP1, dP2, Dr, dD1, dD2 = coef
    per = lambda f: np.asarray(f, dtype=np.float64).reshape(3, -1).T   # noqa: E731
    gabs = cn.readout(np.abs(F), pos, N, L)
    pn = per(cn.kick(F, p1, p2, pres, pos, L, coef, 0)[0])
    b_pres = pc.sum_bound(per(pres), gabs * cK, dP1 * per(p1), dP2 * per(p2)) + pc.storage_bound(pn, dtype)
    b_pos = abs(Dr) * b_pres + pc.sum_bound(pos, pn * Dr, dD1 * per(p1), dD2 * per(p2), np.abs(pos) + 2 * L)
    return b_pres, b_pos


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_kick_readout_on_constructed_forces(N, L, prec):
    s = Stages(N, L, prec)
    pos, m, f = pc.kick_particles(N, L)
    pos[100, 1], m[100, 1], f[100, 1] = -0.0, 0, 0.                      # -0.0 is node 0
    zero = np.zeros((3, N, N, N))
    only_readout = [1., 0., 0., 0., 0., 0.]
    for F, want in ((np.full((3, N, N, N), 3.25), np.full((N ** 3, 3), 3.25)), (pc.linear_force(N), pc.linear_readout(m, f, N))):
        for name, a in (("force", F), ("psi1", zero), ("psi2", zero), ("pres", zero), ("pos", pos)):
            s.put(name, a)
        s.kick(only_readout, 0)
        np.testing.assert_array_equal(s.get("pres").reshape(3, -1).T, want)
        assert s.get("pos").tobytes() == pos.tobytes()                  # drift = 0: untouched, the sign of -0.0 included
    # drift = 1 from the Lagrangian nodes with init's displacements: the same wrap, the same positions
    psi1, psi2, want, _ = pc.init_displacements(N, L)
    for name, a in (("force", zero), ("psi1", psi1), ("psi2", psi2), ("pres", zero), ("pos", cn.lagrangian(N, L))):
        s.put(name, a)
    s.kick([0., 0., 0., 0., 1., 1.], 1)
    moved = s.get("pos")
    np.testing.assert_array_equal(moved, want)
    assert np.all((moved >= 0.) & (moved < L)) and not s.get("pres").any()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_kick_against_the_statement(N, L, prec):
    s = Stages(N, L, prec)
    rs = np.random.RandomState(5 + N)
    F, p1, p2, pres = [_stored(x, prec) for x in rs.normal(size=(4, 3, N, N, N))]
    pos = np.concatenate([pc.tiled_positions(N, L)[:N ** 3 // 2], rs.uniform(-1.5 * L, 2.5 * L, (N ** 3 - N ** 3 // 2, 3))])
    coef = [0.75, 0.3, -0.2, 0.4 * L / N, 1.3, -0.6]
    for drift in (0, 1):
        for name, a in (("force", F), ("psi1", p1), ("psi2", p2), ("pres", pres), ("pos", pos)):
            s.put(name, a)
        s.kick(coef, drift)
        want_pres, want_pos = cn.kick(F, p1, p2, pres, pos, L, coef, drift, DT[prec])
        b_pres, b_pos = _kick_bounds(F, p1, p2, pres, pos, N, L, coef, DT[prec])
        got = s.get("pres").reshape(3, -1).T
        assert np.all(np.abs(got - want_pres.reshape(3, -1).T) <= b_pres)
        new = s.get("pos")
        if drift:
            d = new - want_pos
            d -= L * np.round(d / L)                                    # a rounding may fold across the seam
            assert np.all(np.abs(d) <= b_pos) and np.all((new >= 0.) & (new < L))
        else:
            assert new.tobytes() == pos.tobytes()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_readout_is_the_transpose_of_paint(N, L, prec):
    """sum_p w_p readout(F)_p = sum_nodes F paint(w): the kick's copy of the node arithmetic against fb_paint's.  Bound: the
    sums' (sum_bound over |F| paint(|w|), once for each side) and one rounding of each stored read-out and node."""
    s = Stages(N, L, prec)
    rs = np.random.RandomState(N)
    pos = np.concatenate([pc.tiled_positions(N, L)[:N ** 3 // 2], rs.uniform(-L, 2 * L, (N ** 3 - N ** 3 // 2, 3))])
    F = _stored(rs.normal(size=(3, N, N, N)), prec)
    w = rs.normal(size=N ** 3)
    zero = np.zeros((3, N, N, N))
    for name, a in (("force", F), ("psi1", zero), ("psi2", zero), ("pres", zero), ("pos", pos)):
        s.put(name, a)
    s.kick([1., 0., 0., 0., 0., 0.], 0)
    g = s.get("pres").reshape(3, -1).T
    mesh = _paint(s.box, pos, "cic", w)
    aw = cn.paint(pos, N, L, np.abs(w))
    for c in range(3):
        lhs, rhs = math.fsum(w * g[:, c]), math.fsum((F[c] * mesh).reshape(-1))
        bound = 2 * math.fsum(pc.sum_bound(np.abs(F[c]) * aw).reshape(-1)) \
            + math.fsum(np.abs(w) * pc.storage_bound(g[:, c], DT[prec])) \
            + math.fsum((np.abs(F[c]) * pc.storage_bound(mesh, DT[prec])).reshape(-1))
        assert abs(lhs - rhs) <= bound, (c, lhs - rhs, bound)
        assert abs(lhs) > 1e6 * bound if prec == "f64" else abs(lhs) > 10 * bound


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", COLA_GEOS)
def test_velocity_strides_and_grid_velocity(N, L, prec):
    s = Stages(N, L, prec)
    n3 = N ** 3
    rs = np.random.RandomState(9 + N)
    p1, p2, pres = [_stored(x, prec) for x in rs.normal(size=(3, 3, N, N, N))]
    for name, a in (("psi1", p1), ("psi2", p2), ("pres", pres)):
        s.put(name, a)
    P1, P2, fac = 0.7, -0.35, 123.5
    want = cn.velocity(p1, p2, pres, P1, P2, fac)
    per = lambda f: f.reshape(3, -1).T                                 # noqa: E731
    bound = 2 * abs(fac) * pc.sum_bound(per(pres), P1 * per(p1), P2 * per(p2))
    out = s.eng._alloc_bytes(8 * 3 * n3)
    for stride in (1, 3):
        for c in range(3):
            s.put_at(out.ptr, np.full(3 * n3, -777.), np.float64)
            _lib.call("fb_cola_velocity", s.P, s.ptr("psi1"), s.ptr("psi2"), s.ptr("pres"), c, P1, P2, fac,
                      out.ptr + (8 * c if stride == 3 else 0), stride, s.S)
            h = s.get_at(out.ptr, (3 * n3,), np.float64)
            sel = np.zeros(3 * n3, dtype=bool)
            sel[(c if stride == 3 else 0)::stride][:n3] = True
            if stride == 1:
                sel[n3:] = False
            assert np.all(np.abs(h[sel] - want[:, c]) <= bound[:, c]) and np.all(h[~sel] == -777.), (stride, c)
    # grid velocity: num / count as stored, 0 -- not NaN -- where the count is 0
    count = rs.randint(0, 3, (N, N, N)).astype(np.float64)
    num = _stored(rs.normal(size=(N, N, N)), prec)
    num[0, 0, 0], count[0, 0, 0] = 0., 0.                               # 0 / 0
    s.put("delta", num)
    s.put("count", count)
    _lib.call("fb_cola_grid_velocity", s.P, s.ptr("delta"), s.ptr("count"), s.S)
    gv = s.get("delta")
    ref = cn.grid_velocity(num, count, DT[prec])
    assert np.all(np.isfinite(gv)) and np.all(gv[count == 0.] == 0.) and (count == 0.).sum() > N
    assert np.all(np.abs(gv - ref) <= pc.storage_bound(ref, DT[prec]))


@pytest.mark.parametrize("prec", PRECS)
def test_stage_chain_is_fb_cola_run(prec):
    N, L, n_steps = 16, 32., 2
    s = Stages(N, L, prec)
    tab = cola.launch_table(cola.Growth(s.box.cosmo), 0., 15., n_steps)
    d0 = pc.gaussian_field(N)
    st = s.eng.cola_run(s.eng.upload(d0, REAL), n_steps, tab)
    s.eng.sync()
    run = {"pos": s.get_at(st["pos"].ptr, (N ** 3, 3), np.float64), "pres": s.get_at(st["pres"].ptr, (3, N, N, N), s.dt),
           "delta": s.get_at(st["delta"].ptr, (N, N, N), s.dt)}
    s.lpt(d0)
    s.put("pres", np.full((3, N, N, N), 7.))
    s.init(tab[0], tab[1])
    for j in range(n_steps + 1):
        s.force(tab[2])
        s.kick(tab[3 + 6 * j: 9 + 6 * j], j < n_steps)
    for name in ("pos", "pres", "delta"):
        assert s.get(name, raw=True).tobytes() == run[name].tobytes(), name
    assert np.std(run["delta"].astype(np.float64)) > 1e-3 and np.all((run["pos"] >= 0.) & (run["pos"] < L))
