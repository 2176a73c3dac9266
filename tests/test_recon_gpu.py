"""GPU: density-field reconstruction and mesh readout (fb_recon.hip; CosmoBox.reconstruct, .readout, .uniform_catalogue) on the
constructed cases of tests/recon_cases.py, in both precisions, stage by stage against the numpy statement of
tests/recon_numpy.py -- which tests/test_recon_cases_cpu.py validates on its own -- each stage fed the statement's exact inputs so
that errors do not compound.  Nothing is larger than 32^3; most cases run at 16^3 and 18^3."""
import ctypes
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, DeviceArray, _lib, default_cosmo, recon
from fastbox_amd import rng as fb_rng
from fastbox_amd.device import HALF
from fastbox_amd.halos import HaloCatalogue
from tests import recon_cases as rc
from tests import recon_numpy as rn

pytestmark = pytest.mark.gpu
PRECS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
PSI_TOL = {"f64": 1e-11, "f32": 1e-5}          # of max|Psi|: the project's parity tolerances for transformed fields (README)
GEOMS = rc.geometries()
GEOM_IDS = ["N%d-%s" % (N, "x".join("%g" % a for a in L)) for N, L in GEOMS]
READ_GEOMS, READ_IDS = GEOMS[1:], GEOM_IDS[1:]  # the cuboid 16^3 and 18^3
SEED = 3


@functools.lru_cache(maxsize=None)
def _box(prec, N, L):
    return CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=prec, rng="device", seed=SEED)


def _upload_half(eng, spec):
    """A half spectrum (N, N, N/2 + 1) as the device stores it: (N, rows, pitch), padding zero."""
    N = eng.N
    raw = np.zeros((N, eng.rows, eng.pitch), dtype=eng.cdtype)
    raw[:, :N, :N // 2 + 1] = spec
    d = eng.empty(HALF)
    _lib.call("fb_memcpy_h2d", d.ptr, raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes, eng.stream)
    eng.sync()
    return d


def _catalogue(box, pos):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    return HaloCatalogue(box.engine, box.engine.upload_raw(pos) if pos.shape[0] else None, pos.shape[0])


def _densities(N, L):
    out = {name: rc.plane_wave(N, L, mode)[0] for name, mode in rc.WAVES.items()}
    out["random"] = rc.random_field(N)
    return out


# ---- displacement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS, ids=GEOM_IDS)
def test_displacement_is_the_statement(N, L, prec):
    """Plane waves (along x, along z, oblique) and a random field: max error <= 1e-11 (fp64 plan) / 1e-5 (f32 plan) of max|Psi|,
    from the statement's own delta(k) uploaded as a half spectrum; and once through the device's own r2c of the real field."""
    box, dt = _box(prec, N, L), DT[prec]
    R, b, beta = rc.PARAMS["R"], rc.PARAMS["b"], rc.PARAMS["beta"]
    for name, delta in sorted(_densities(N, L).items()):
        dk = rn.rfftn(rn.stored(delta, dt), dt)
        want = rn.displacement_k(dk, L, R, b, beta, dt)
        got = np.array([np.asarray(p) for p in recon.displacement(box, _upload_half(box.engine, dk), R, b, f=beta * b)])
        scale = np.max(np.abs(want))
        err = np.max(np.abs(got - want)) / scale
        print("%s, %s, N = %d, L = %s: max error %.3e of max|Psi| = %.3e" % (name, prec, N, L, err, scale))
        assert scale > 1e-3 and err <= PSI_TOL[prec]
        if name == "oblique":
            wave = rc.plane_wave_psi(N, L, rc.WAVES[name], R, b, beta)
            assert np.max(np.abs(got - wave)) <= PSI_TOL[prec] * scale
    got = np.array([np.asarray(p) for p in recon.displacement(box, delta, R, b, f=beta * b)])     # the random field, r2c on the device
    err = np.max(np.abs(got - want)) / scale
    print("random through r2c, %s: max error %.3e" % (prec, err))
    assert err <= PSI_TOL[prec]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", GEOMS[1:], ids=GEOM_IDS[1:])
def test_displacement_is_zero_on_its_own_nyquist_plane_and_at_k0(N, L, prec):
    box = _box(prec, N, L)
    for axis in range(3):
        spec, _ = rc.nyquist_mode_spectrum(N, axis)
        psi = [np.asarray(p) for p in recon.displacement(box, _upload_half(box.engine, spec), 3., 1., f=0.3)]
        assert np.all(psi[axis] == 0.)
        if axis < 2:                                        # (an interior k_z: the other two components are there)
            assert all(np.max(np.abs(psi[c])) > 0. for c in range(3) if c != axis)
    spec = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    spec[0, 0, 0] = 5.
    assert all(np.all(np.asarray(p) == 0.) for p in recon.displacement(box, _upload_half(box.engine, spec), 3., 1., f=0.3))


# ---- readout and shift ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", rc.WINDOWS)
@pytest.mark.parametrize("N,L", READ_GEOMS, ids=READ_IDS)
def test_readout_is_the_statement(N, L, window, prec):
    """Nodes, midpoints, the seam (0, just below L, L, negative inputs that wrap), n = 1, 257 and 0; three fields, two and one.
    Bound 64 * 2^-53 * max|F| on both plans, the field rounded to the plan's precision beforehand (recon_cases readout_bound)."""
    box, dt = _box(prec, N, L), DT[prec]
    F = np.concatenate([rc.readout_fields(N)[:2], rc.random_field(N)[None]])
    Fs = rn.stored(F, dt)
    bound = rc.readout_bound(F, dt)
    for name, pos in sorted(rc.readout_positions(N, L).items()):
        got = box.readout(list(F), pos, window=window)
        assert isinstance(got, recon.DeviceValues) and got.shape == (pos.shape[0], 3)
        got = np.asarray(got)
        want = rn.readout(Fs, pos, L, window)
        err = np.max(np.abs(got - want)) if pos.shape[0] else 0.
        print("%s, %s, %s, N = %d: max error %.3e, bound %.3e" % (name, window, prec, N, err, bound))
        assert got.dtype == np.float64 and not np.any(np.isnan(got)) and err <= bound
    pos = rc.readout_positions(N, L)["wave tail"]
    cat = _catalogue(box, pos)
    one = box.readout(box.engine.upload(F[2], "real"), cat, window=window)
    assert one.shape == (pos.shape[0],)
    np.testing.assert_array_equal(np.asarray(one), np.asarray(box.readout(list(F), cat, window=window))[:, 2])
    two = np.asarray(box.readout([F[1], F[2]], cat, window=window))
    assert two.shape == (pos.shape[0], 2) and np.max(np.abs(two - rn.readout(Fs[1:], pos, L, window))) <= bound


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", READ_GEOMS, ids=READ_IDS)
def test_readout_on_nodes_is_exact(N, L, prec):
    """NGP and CIC return the node's value itself; TSC its (1/8, 3/4, 1/8)^3 stencil, exact for these dyadic fields."""
    box = _box(prec, N, L)
    F = rc.readout_fields(N)                                 # exact in f32
    pos, idx = rc.node_positions(N, L)
    for window in rc.WINDOWS:
        got = np.asarray(box.readout(list(F), pos, window=window))
        for c in range(3):
            want = F[c][idx[:, 0], idx[:, 1], idx[:, 2]] if window != "tsc" else rc.tsc_node_stencil(F[c], idx)
            np.testing.assert_array_equal(got[:, c], want)
    for window in rc.WINDOWS:                                # a constant reads as the constant: the weights sum to 1
        const = np.asarray(box.readout(np.full((N, N, N), 2.75), pos + 0.3, window=window))
        assert const.shape == (pos.shape[0],) and np.max(np.abs(const - 2.75)) <= 8 * 2. ** -53 * 2.75


def _shift_bound(psi, pos, L, scale, scale_z, dt):
    """|got - want| modulo L per axis: (|scale| + |scale_z|) times the readout bound, plus four roundings of numbers no larger
    than |x| + |d| + L (the products scale Psi, their sum, x - d and the wrap's x - L floor(x / L)); the kernel's operations are
    the statement's in the statement's order, so the difference is expected to be 0."""
    d = (abs(scale) + abs(scale_z)) * float(np.max(np.abs(psi)))
    return (abs(scale) + abs(scale_z)) * rc.readout_bound(psi, dt) + 4 * 2. ** -53 * (float(np.max(np.abs(pos))) + d + max(L))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("window", rc.WINDOWS)
@pytest.mark.parametrize("N,L", READ_GEOMS, ids=READ_IDS)
def test_shift_is_the_statement(N, L, window, prec):
    box, dt = _box(prec, N, L), DT[prec]
    cell = np.asarray(L) / N
    psi = (rc.readout_fields(N) - 1.) * (1.5 * cell).reshape(3, 1, 1, 1)         # a few cells, both signs
    psis = rn.stored(psi, dt)
    La = np.asarray(L)
    for name, pos in sorted(rc.readout_positions(N, L).items()):
        for scale, scale_z in ((1., 0.), (1., 0.5), (-2., 1.)):
            got = recon.displace_catalogue(box, list(psi), pos, window=window, scale=scale, scale_z=scale_z)
            assert isinstance(got, HaloCatalogue) and got.n == pos.shape[0]
            got = np.asarray(got)
            want = rn.shift(psis, pos, L, window, scale, scale_z)
            assert got.shape == want.shape
            if not pos.shape[0]:
                continue
            assert np.all((got >= 0.) & (got < La))
            diff = np.abs(got - want)
            err = np.max(np.minimum(diff, La - diff))
            bound = _shift_bound(psi, pos, L, scale, scale_z, dt)
            print("%s, %s, %s, N = %d, scales (%g, %g): max error %.3e, bound %.3e" % (name, window, prec, N, scale, scale_z, err, bound))
            assert err <= bound


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", READ_GEOMS, ids=READ_IDS)
def test_shift_by_nothing_wraps_and_in_place_is_the_same(N, L, prec):
    """Psi = 0 returns the wrapped input positions bit for bit; pos_out aliasing pos_in gives the bits of not aliasing; the
    gather from the interleaved copy (N^3 / 8 particles or more) gives the bits of the gather from the three fields."""
    box = _box(prec, N, L)
    sets = rc.readout_positions(N, L)
    few, many = np.concatenate([sets["seam"], sets["wave tail"]]), sets["crowd"]
    assert few.shape[0] < N ** 3 // rc.STAGE_DIV <= many.shape[0]
    zero = [np.zeros((N, N, N))] * 3
    cell = np.asarray(L) / N
    psi = list((rc.readout_fields(N) - 1.) * (1.5 * cell).reshape(3, 1, 1, 1))
    for pos in (few, many):
        for window in rc.WINDOWS:
            np.testing.assert_array_equal(np.asarray(recon.displace_catalogue(box, zero, pos, window=window, scale=1., scale_z=0.5)),
                                          rn.wrap(pos, L))
        apart = np.asarray(recon.displace_catalogue(box, psi, _catalogue(box, pos), scale=1., scale_z=0.5))
        cat = _catalogue(box, pos)
        same = recon.displace_catalogue(box, psi, cat, scale=1., scale_z=0.5, inplace=True)
        assert same is cat
        np.testing.assert_array_equal(np.asarray(same), apart)
        assert not np.array_equal(apart, rn.wrap(pos, L))
    both = np.asarray(recon.displace_catalogue(box, psi, many, window="tsc", scale=-1., scale_z=0.25))
    for lo in range(0, many.shape[0], few.shape[0]):                        # the same particles in pieces below the threshold
        piece = many[lo:lo + few.shape[0]]
        np.testing.assert_array_equal(np.asarray(recon.displace_catalogue(box, psi, piece, window="tsc", scale=-1., scale_z=0.25)),
                                      both[lo:lo + few.shape[0]])


# ---- random and grid positions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 1000, 4099))
def test_uniform_positions_are_the_host_model(n):
    N, L = GEOMS[1]
    box = _box("f32", N, L)
    cat = box.uniform_catalogue(n, seed=77)
    assert isinstance(cat, HaloCatalogue) and cat.n == n and (cat.seed, cat.realisation) == (77, 0)
    np.testing.assert_array_equal(np.asarray(cat), fb_rng.recon_uniforms(n, L, 77, 0))
    nxt = box.uniform_catalogue(n)                                          # the box's seed, its next draw
    np.testing.assert_array_equal(np.asarray(nxt), fb_rng.recon_uniforms(n, L, nxt.seed, nxt.realisation))
    assert nxt.seed == SEED and box.uniform_catalogue(n).realisation == nxt.realisation + 1
    assert box.uniform_catalogue(0).n == 0


def test_grid_nodes_are_the_statement():
    N, L = GEOMS[1]
    np.testing.assert_array_equal(np.asarray(recon.grid_catalogue_nodes(_box("f64", N, L))), rn.grid_positions(N, L))


# ---- reconstruct end to end ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _physical(f):
    return rc.physical_case(f)


@functools.lru_cache(maxsize=None)
def _statement(f, randoms, prec):
    c = _physical(f)
    N, L = c["N"], c["L"]
    R = rn.grid_positions(N, L) if randoms == "grid" else rn.uniform_positions(4 * N ** 3, L, SEED, 0)
    out = rn.reconstruct(c["data"], R, N, L, c["R"], 1., f, dtype=DT[prec])
    return rn.cross_correlation(out["delta_rec"], c["delta_lin"], L)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("randoms", ("grid", "drawn"))
@pytest.mark.parametrize("f", (0., 0.5))
def test_reconstruct_end_to_end(f, randoms, prec):
    """32^3, the CPU-validated physical case: delta_rec is bitwise repeatable and independent of the order of the data; r(k) with
    the linear field is within 0.02 of the statement's in every bin and above the unreconstructed r(k) in every bin."""
    c = _physical(f)
    N, L = c["N"], c["L"]
    box = _box(prec, N, L)
    kw = dict(randoms="grid" if randoms == "grid" else None, smoothing=c["R"], bias=1., f=f, convention="sym")
    rec = box.reconstruct(c["data"], **kw)
    assert isinstance(rec, recon.Reconstruction) and isinstance(rec.delta_rec, DeviceArray)
    assert (rec.n_data, rec.n_random) == (N ** 3, N ** 3 if randoms == "grid" else 4 * N ** 3)
    assert (rec.smoothing, rec.bias, rec.f, rec.convention, rec.displacement) == (c["R"], 1., f, "sym", None)
    got = np.asarray(rec.delta_rec)
    np.testing.assert_array_equal(np.asarray(box.reconstruct(c["data"], **kw).delta_rec), got)
    perm = np.random.RandomState(1).permutation(N ** 3)
    again = box.reconstruct(c["data"][perm], **kw)
    np.testing.assert_array_equal(np.asarray(again.delta_rec), got)
    np.testing.assert_array_equal(np.asarray(again.data), np.asarray(rec.data)[perm])
    after = rn.cross_correlation(got, c["delta_lin"], L)
    before = rn.cross_correlation(np.asarray(recon.density_contrast(box, c["data"])), c["delta_lin"], L)
    want = _statement(f, randoms, prec)
    print("f = %g, %s randoms, %s: r(k) before %s after %s statement %s" % (f, randoms, prec, np.round(before, 3), np.round(after, 3),
                                                                             np.round(want, 3)))
    assert np.max(np.abs(after - want)) <= 0.02
    assert np.all(after > before)


@pytest.mark.parametrize("prec", PRECS)
def test_reconstruct_conventions_delta_and_displacement(prec):
    """'iso' differs from 'sym' in the randoms only; ``delta=`` with the data's own painted density reproduces the default path
    bit for bit; the displacement returned is the stage's; catalogues and host arrays are the same input."""
    c = _physical(0.5)
    N, L = c["N"], c["L"]
    box = _box(prec, N, L)
    kw = dict(randoms="grid", smoothing=c["R"], bias=1., f=0.5)
    sym = box.reconstruct(c["data"], convention="sym", return_displacement=True, **kw)
    iso = box.reconstruct(c["data"], convention="iso", **kw)
    np.testing.assert_array_equal(np.asarray(sym.data), np.asarray(iso.data))
    rs, ri = np.asarray(sym.randoms), np.asarray(iso.randoms)
    np.testing.assert_array_equal(rs[:, :2], ri[:, :2])
    assert not np.array_equal(rs[:, 2], ri[:, 2]) and not np.array_equal(np.asarray(sym.delta_rec), np.asarray(iso.delta_rec))
    delta = recon.density_contrast(box, c["data"])
    given = box.reconstruct(c["data"], convention="sym", delta=delta, **kw)
    np.testing.assert_array_equal(np.asarray(given.delta_rec), np.asarray(sym.delta_rec))
    np.testing.assert_array_equal(np.asarray(given.data), np.asarray(sym.data))
    psi = recon.displacement(box, delta, c["R"], 1., f=0.5)
    assert len(sym.displacement) == 3
    for a in range(3):
        np.testing.assert_array_equal(np.asarray(sym.displacement[a]), np.asarray(psi[a]))
    cat = _catalogue(box, c["data"])
    rand = _catalogue(box, rn.grid_positions(N, L))
    both = box.reconstruct(cat, randoms=rand, smoothing=c["R"], bias=1., f=0.5)
    np.testing.assert_array_equal(np.asarray(both.delta_rec), np.asarray(sym.delta_rec))
    np.testing.assert_array_equal(np.asarray(rand), rn.grid_positions(N, L))            # a caller's randoms are not moved
    some = box.reconstruct(cat, randoms=5000, seed=12, smoothing=c["R"])
    assert some.n_random == 5000
    moved = recon.displace_catalogue(box, list(recon.displacement(box, recon.density_contrast(box, cat), c["R"])),
                                     fb_rng.recon_uniforms(5000, L, 12, 0))
    np.testing.assert_array_equal(np.asarray(some.randoms), np.asarray(moved))


def test_reconstructed_xi_is_landy_szalay_of_the_three_counts():
    c = _physical(0.)
    N, L = c["N"], c["L"]
    box = _box("f32", N, L)
    some = np.sort(np.random.RandomState(6).permutation(N ** 3)[:4096])
    rec = box.reconstruct(c["data"][some], randoms=8192, smoothing=c["R"])
    edges = np.linspace(2., 12., 6)
    r, xi = recon.reconstructed_xi(box, rec, edges)
    dd, ds, ss = box.pair_counts(rec.data, edges=edges), box.pair_counts(rec.data, rec.randoms, edges=edges), \
        box.pair_counts(rec.randoms, edges=edges)
    np.testing.assert_array_equal(r, 0.5 * (edges[1:] + edges[:-1]))
    np.testing.assert_allclose(xi, (dd.xi + 1.) - 2. * (ds.xi + 1.) + (ss.xi + 1.), rtol=0, atol=1e-12)
    assert xi.shape == (5,) and np.all(np.isfinite(xi))


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(monkeypatch):
    N, L = GEOMS[1]
    box = _box("f32", N, L)
    pos = rc.readout_positions(N, L)["wave tail"]
    for bad in (np.nan, np.inf, 2. ** 53 * L[0]):
        p = pos.copy()
        p[5, 0] = bad
        with pytest.raises(ValueError, match="data"):
            box.reconstruct(p)
        with pytest.raises(ValueError, match="data"):
            box.reconstruct(_catalogue(box, p))
        with pytest.raises(ValueError, match="randoms"):
            box.reconstruct(pos, randoms=p)
        with pytest.raises(ValueError, match="positions"):
            box.readout(np.zeros((N, N, N)), p)
    for kw, name in ((dict(smoothing=0.), "smoothing"), (dict(smoothing=-1.), "smoothing"), (dict(smoothing=np.nan), "smoothing"),
                     (dict(bias=0.), "bias"), (dict(f=-0.1), "f"), (dict(convention="both"), "convention"),
                     (dict(window="pcs"), "window"), (dict(randoms="lattice"), "randoms"), (dict(randoms=0), "randoms")):
        with pytest.raises(ValueError, match=name):
            box.reconstruct(pos, **kw)
    with pytest.raises(ValueError, match="data"):
        box.reconstruct(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="data"):
        box.reconstruct(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="window"):
        box.readout(np.zeros((N, N, N)), pos, window="pcs")
    with pytest.raises(ValueError, match="field"):
        box.readout([np.zeros((N, N, N))] * 4, pos)
    with pytest.raises(TypeError, match="delta"):
        box.reconstruct(pos, delta=np.zeros((N, N, N), dtype=np.complex128))
    with pytest.raises(TypeError, match="delta"):
        box.reconstruct(pos, delta=box.engine.empty("full"))
    with pytest.raises(ValueError, match="n"):
        box.uniform_catalogue(-1)
    assert box.engine.free_bytes() > box.engine.lib.fb_recon_work_bytes(box.engine._plan, pos.shape[0], 4 * pos.shape[0]) > 0
    monkeypatch.setattr(box.engine, "free_bytes", lambda: 1 << 10)
    with pytest.raises(MemoryError, match="work memory"):
        box.reconstruct(pos)
