"""CPU: the constructed cases of tests/particle_cases.py against the numpy statements (tests/halos_numpy.py, tests/cola_numpy.py)
and the host model of the Poisson draw (fastbox_amd/rng.py), and for every case the property that keeps it from being vacuous:
the top class really reaches 2^24, the tables really take the other path, the seam cases really wrap.
tests/test_particle_edges_gpu.py holds the device to the same cases."""
import math

import numpy as np
import pytest

from fastbox_amd import cola, rng
from fastbox_amd.cosmology import Cosmology
from tests import cola_numpy as cn
from tests import halos_numpy as hn
from tests import particle_cases as pc

F32, F64 = np.float32, np.float64


def _same_in_fp32(x):
    return np.array_equal(np.asarray(x, dtype=F64).astype(F32).astype(F64), x)


# ---- 1. expected counts and the Poisson draw ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 32])
def test_poisson_box_spans_the_range(N):
    b = pc.poisson_box(N)
    lam = hn.expected_counts(b["delta"], b["nbar"], b["bias"], b["L"])
    assert _same_in_fp32(b["delta"]) and np.array_equal(lam, b["nbar"] * (1. + b["delta"]))
    assert lam.max() == pc.LAM_MAX == lam[b["top"]] and lam.min() > 0. and lam.min() < 1.2e-300
    assert np.sum(lam > 0.99 * pc.LAM_MAX) > N * N // 64                       # the top class really reaches 2^24
    row = lam[b["int_row"]]
    assert np.array_equal(row, np.floor(row)) and np.all(row >= 1.) and row.max() > 1.5e7
    assert np.unique(row).size >= N - 4                                 # one integer per class (1e-300 .. 1 share the 1)
    for iz, c in enumerate(b["classes"]):                               # every class is spread by +-10 %
        l = np.delete(lam[:, :, iz].reshape(-1), [b["int_row"][0] * N + b["int_row"][1]])
        if (b["top"][2] == iz):
            l = l[l != pc.LAM_MAX]
        assert 0.9 * c <= l.min() < 0.92 * c and 1.08 * c < l.max() <= 1.1 * c
    assert np.all(np.diff(b["classes"]) > 0) and b["classes"][-1] * 1.1 <= pc.LAM_MAX * (1 + 1e-15)


def test_host_model_brackets_its_uniform():
    """rng.poisson_inverse on the 16^3 box: every count brackets its uniform in scipy's CDF within 8 units.  Measured here: none needed (0.000
    units); 0 voxels of 4096 differ from poisson.ppf.  A count that is off by one is outside the bracket in all but a few voxels
    of the top classes."""
    N, seed, real = 16, 7, 3
    b = pc.poisson_box(N)
    lam = hn.expected_counts(b["delta"], b["nbar"], b["bias"], b["L"])
    u = rng.poisson_uniforms(N ** 3, seed, real)
    k = rng.stream_poisson(lam, seed, real).reshape(-1)
    slack, nppf = pc.poisson_bracket(k, lam, u)
    print("host model: slack %.3f units, %d voxels differ from ppf" % (slack, nppf))
    assert slack <= 8., (slack, nppf)
    assert nppf <= 4
    assert k[np.ravel_multi_index(b["top"], lam.shape)] > 1.6e7 and k.max() < 2 ** 25
    # sensitivity: +-1 leaves the bracket wherever the pmf is above the slack
    from scipy.stats import poisson
    for d in (-1., 1.):
        kk = np.maximum(k + d, 0.)
        need = np.maximum(poisson.cdf(kk - 1., lam.reshape(-1)) - u, u - poisson.cdf(kk, lam.reshape(-1)))
        caught = need > 8. * pc.poisson_unit(lam.reshape(-1))
        assert caught[kk != k].mean() > 0.99


def test_poisson_unit():
    assert pc.poisson_unit(1e-300) == 2. ** -52 == pc.poisson_unit(1.) == pc.poisson_unit(0.5)
    assert pc.poisson_unit(2. ** 24) == 2. ** -52 * 2. ** 24 * math.log(2. ** 24)


def test_overflow_boxes_have_one_voxel_above():
    N = 32
    b = pc.poisson_box(N)
    boxes = pc.overflow_boxes(N)
    assert len(boxes) == 4
    for name, vox, nbar, delta in boxes:
        lam = hn.expected_counts(delta, nbar, 1., b["L"])
        over = np.argwhere(lam > pc.LAM_MAX)
        assert over.shape[0] == 1 and tuple(over[0]) == tuple(vox), name
        # (the statement's nan_to_num turns +inf into the largest double)
        assert lam[vox] == (pc.LAM_MAX * (1 + 2. ** -20) if name.startswith("above") else np.finfo(F64).max), name
        assert not name.startswith("above") or np.float32(lam[vox]) > np.float32(pc.LAM_MAX)   # fp32 sees the step
        flat = int(np.ravel_multi_index(vox, lam.shape))
        assert flat == N ** 3 - 1 or flat % 64 == 37
        at_limit = nbar.copy()
        at_limit[vox] = pc.LAM_MAX                                      # the limit itself at the same voxel: nothing above
        lam = hn.expected_counts(delta, at_limit, 1., b["L"])
        assert lam[vox] == pc.LAM_MAX == lam.max()


def test_a_draw_above_the_limit_that_fp32_cannot_hold():
    """The voxel with lam = 2^24 draws 2^24 + 811 at particle_cases.ODD_DRAW: odd, so fp32 holds 2^24 + 812 instead."""
    N = 32
    b = pc.poisson_box(N)
    seed, real = pc.ODD_DRAW
    flat = int(np.ravel_multi_index(b["top"], (N, N, N)))
    k = rng.poisson_inverse(np.array([pc.LAM_MAX]), rng.poisson_uniforms(1, seed, real, first=flat))[0]
    assert k == 2 ** 24 + 811 and np.float32(k) == 2 ** 24 + 812


def test_lognormal_box_and_shift_sensitivity():
    N = 32
    delta, bias = pc.lognormal_box(N)
    assert _same_in_fp32(delta) and (bias * delta).max() == 30. and (bias * delta).min() == -30.
    ref, shifted = pc.lognormal_statements(delta, bias, (float(N),) * 3)
    assert np.all(np.isfinite(ref)) and ref.max() > 50. * ref.mean() and ref.min() < 1e-12
    dref = pc.lognormal_deviation(shifted, ref, 1.)
    assert 0. < dref < 1e-13                                          # the bound of the GPU test is the 1e-13 floor or 10 dref


def test_field_params_see_an_index_error():
    N = 32
    delta, nbar, bias = pc.field_params(N)
    nbar, bias, delta = [np.broadcast_to(a, (N, N, N)).copy() for a in (nbar, bias, delta)]
    assert all(_same_in_fp32(a) for a in (nbar, bias, delta))
    lam = hn.expected_counts(delta, nbar, bias, (64., 64., 64.))
    assert lam.min() > 0.
    for perm in ((1, 0, 2), (0, 2, 1), (2, 1, 0)):
        assert not np.array_equal(hn.expected_counts(delta, nbar.transpose(perm), bias, (64.,) * 3), lam)
        assert not np.array_equal(hn.expected_counts(delta, nbar, bias.transpose(perm), (64.,) * 3), lam)


# ---- 2. catalogue tables ------------------------------------------------------------------------------------------------------
def test_catalogue_cases_take_their_paths():
    N, n = 64, 64 ** 3
    c = pc.catalogue_counts("atomic")
    big = np.argwhere(c >= pc.LDS_COUNTS)
    assert pc.table_layout(n, int(c.max())) == (4096, 64, 79) and c.max() == 5000
    assert len({int(i[0]) for i in big}) >= 5 and (c == 4095).sum() == 1          # several tiles; the largest LDS count
    flat = np.ravel_multi_index(big.T, c.shape)
    steps = {}
    for f, v in zip(flat, c.reshape(-1)[flat]):
        steps.setdefault((int(f) // 256, int(v)), []).append(int(f))
    assert len(steps[(41 * 16, 5000)]) == 2 and len(steps[(41 * 16, 4096)]) == 2  # same count, same 256-voxel step
    assert (41 * 16 + 10, 5000) in steps and c.reshape(-1)[-1] == 5000
    c = pc.catalogue_counts("carry")
    tile, tiles, chunks = pc.table_layout(n, int(c.max()))
    assert (tile, tiles, chunks) == (4096, 64, 313) and (c.max() + 1) * tiles > 2 ** 20 and chunks > 256
    c = pc.catalogue_counts("doubling")
    tile, tiles, chunks = pc.table_layout(n, int(c.max()))
    assert (tile, tiles) == (8192, 32) and (c.max() + 1) * 64 > 2 ** 25 >= (c.max() + 1) * 32
    assert pc.table_layout(n, 524287)[:2] == (4096, 64) and pc.table_layout(n, 524288)[:2] == (8192, 32)   # the threshold
    f = int(np.argmax(c))
    assert f % 8192 == 8191 and f // 4096 == 5                          # last voxel of the doubled tile 2, of the old tile 5
    for name in ("atomic", "carry", "doubling"):
        c = pc.catalogue_counts(name)
        cat = hn.catalogue(c, (640., 650., 660.))
        assert cat.shape == (c.sum(), 3)
        assert np.array_equal(cat[-1] / (np.array((640., 650., 660.)) / N), np.unravel_index(int(np.argmax(c == c.max())
                                                                                                if name != "atomic" else n - 1),
                                                                                           c.shape))


# ---- 3. painting --------------------------------------------------------------------------------------------------------------
def _paints(pos, N, L, window, weights=None):
    """Every numpy statement that covers the case: halos_numpy.paint and, for CIC on a cubic box, cola_numpy.paint."""
    out = [hn.paint(pos, N, L, window, weights)]
    ok = np.all(np.isfinite(pos), axis=1)
    if window == "cic" and L[0] == L[1] == L[2] and ok.all():
        out.append(cn.paint(np.asarray(pos, dtype=F64), N, L[0], None if weights is None else np.asarray(weights, dtype=F64)))
    return out


@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", pc.paint_geometries())
def test_paint_known_weights(N, L, window):
    pos, labels = pc.paint_positions(N, L)
    assert len(labels) == pos.shape[0] == 4 + 3 * len(pc.SEAM)
    u = pos / (np.asarray(L) / N)
    assert (u < 0).any() and (u >= N).any() and np.any(u == N) and np.any(np.signbit(u) & (u == 0))   # the seam cases wrap
    w = np.arange(1., pos.shape[0] + 1.)                                # a different weight each: a misplaced particle shows
    want = pc.expected_mesh(pos, N, L, window, w)
    assert want.sum() == w.sum() and want[0].any() and want[:, 0].any() and want[:, :, 0].any()
    assert want[N - 1].any() and want[:, N - 1].any() and want[:, :, N - 1].any()
    for got in _paints(pos, N, L, window, w):
        np.testing.assert_array_equal(got, want)
    # the written-down weights, one particle at a time
    cell = np.asarray(L) / N
    per_axis = {"node": {"ngp": {3: 1.}, "cic": {3: 1.}, "tsc": {2: .125, 3: .75, 4: .125}},
                "mid": {"ngp": {5: 1.}, "cic": {4: .5, 5: .5}, "tsc": {4: .5, 5: .5}},
                "seam mid": {"ngp": {0: 1.}, "cic": {N - 1: .5, 0: .5}, "tsc": {N - 1: .5, 0: .5}},
                "seam node": {"ngp": {0: 1.}, "cic": {0: 1.}, "tsc": {N - 1: .125, 0: .75, 1: .125}}}
    for name, us in (("node", [3.]), ("mid", [4.5]), ("seam mid", [N - .5, -.5]), ("seam node", [0., -0., float(N), 4. * N])):
        for uu in us:
            line = pc.expected_mesh(np.array([[uu, 3., 3.]]) * cell, N, L, "ngp")[:, 3, 3] if window == "ngp" else \
                pc.expected_mesh(np.array([[uu, 3., 3.]]) * cell, N, L, window).sum(axis=(1, 2))
            tab = np.zeros(N)
            for m, v in per_axis[name][window].items():
                tab[m] = v
            np.testing.assert_array_equal(line, tab, err_msg="%s %s" % (name, uu))


@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", pc.paint_geometries())
def test_paint_just_below_zero(N, L, window):
    pos, at0 = pc.below_zero_positions(N, L)
    assert np.all((pos < 0).sum(axis=1) == 1)
    exact = pc.expected_mesh(pos, N, L, window)
    for got, ref in zip(_paints(pos, N, L, window), _paints(at0, N, L, window)):
        np.testing.assert_array_equal(got, ref)                         # 1 - 2^-60 is 1: the particle at +0
        assert np.max(np.abs(got - exact)) <= 2. ** -52
    np.testing.assert_array_equal(_paints(at0, N, L, window)[0], pc.expected_mesh(at0, N, L, window))


@pytest.mark.parametrize("window", pc.WINDOWS)
def test_paint_totals_are_exact(window):
    N, L = pc.paint_geometries()[1]
    n = 200
    pos = pc.dyadic_cloud(N, L, n, 21)
    sets = pc.weight_sets(n)
    assert sets["zero sum"][0].sum() == 0. and np.abs(sets["zero sum"][0]).sum() > n
    assert pc.paint_exponent(sets["span 2^40"][0], n) == 18 and pc.paint_exponent(None, n) == 53
    for name, (w, total) in sets.items():
        want, exact = pc.expected_mesh(pos, N, L, window, w, return_exact=True)
        assert exact == (name != "span 2^40" or window != "tsc")        # 2^40 beside shares of 2^-21: 61 bits
        got = hn.paint(pos, N, L, window, w)
        if exact:
            np.testing.assert_array_equal(got, want, err_msg=name)
            assert math.fsum(want.reshape(-1)) == total == math.fsum(got.reshape(-1)), name
        else:
            assert np.all(np.abs(got - want) <= 8 * 2. ** -53 * np.abs(want))
            assert abs(math.fsum(want.reshape(-1)) - total) <= 2. ** -53 * np.abs(want).sum()


def test_paint_one_node():
    N, L = pc.paint_geometries()[0]
    node = (N - 1, 0, 5)
    pos = np.tile(np.array(node) * (np.asarray(L) / N), (2 ** 20, 1))
    for wgt, total in ((None, 2. ** 20), (np.full(2 ** 20, 2. ** 30), 2. ** 50)):
        for window in ("ngp", "cic"):
            got = hn.paint(pos, N, L, window, wgt)
            assert got[node] == total and np.count_nonzero(got) == 1
    one = pc.expected_mesh(pos[:1], N, L, "tsc")
    assert one[node] == 27. / 64. and one[0, 0, 5] == 9. / 128. and np.count_nonzero(one) == 27
    assert _same_in_fp32(one * 2. ** 50)


@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", pc.paint_geometries())
def test_paint_translation_and_reflection(N, L, window):
    n = 300
    cell = np.asarray(L) / N
    pos = pc.dyadic_cloud(N, L, n, 33, ties=(window != "ngp"))
    w = pc.weight_sets(n, seed=6)["signed"][0]
    base = hn.paint(pos, N, L, window, w)
    np.testing.assert_array_equal(base, pc.expected_mesh(pos, N, L, window, w))
    shift = np.array([3, -N - 2, 2 * N + 1])
    np.testing.assert_array_equal(hn.paint(pos + shift * cell, N, L, window, w), np.roll(base, shift, axis=(0, 1, 2)))
    np.testing.assert_array_equal(hn.paint(np.asarray(L) - pos, N, L, window, w), pc.reflect_mesh(base))
    assert not np.array_equal(pc.reflect_mesh(base), base)
    if window == "ngp":
        # the tie: a particle on a midpoint belongs to the upper node, and so does its mirror image -- which is the mirror
        # image of the lower node.  NGP is reflection symmetric only away from the midpoints.
        tie = np.array([[4.5, 3., 3.]]) * cell
        a, b = hn.paint(tie, N, L, "ngp"), hn.paint(np.asarray(L) - tie, N, L, "ngp")
        assert a[5, 3, 3] == 1. and b[N - 4, N - 3, N - 3] == 1. and pc.reflect_mesh(a)[N - 5, N - 3, N - 3] == 1.


@pytest.mark.parametrize("window", pc.WINDOWS)
def test_paint_skips_non_finite_and_empty(window):
    N, L = pc.paint_geometries()[1]
    pos = pc.dyadic_cloud(N, L, 60, 44)
    w = np.arange(1., 61.)
    bad = pos.copy()
    rows = [2, 11, 30, 31, 59]
    for r, (a, v) in zip(rows, [(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (2, np.nan)]):
        bad[r, a] = v
    keep = np.setdiff1d(np.arange(60), rows)
    want = pc.expected_mesh(pos[keep], N, L, window, w[keep])
    np.testing.assert_array_equal(hn.paint(bad, N, L, window, w), want)
    np.testing.assert_array_equal(pc.expected_mesh(bad, N, L, window, w), want)
    assert want.sum() == w[keep].sum() != w.sum()
    assert not hn.paint(np.zeros((0, 3)), N, L, window).any()


@pytest.mark.parametrize("window", pc.WINDOWS)
@pytest.mark.parametrize("N,L", pc.paint_geometries())
def test_compensated_spike_spectrum(N, L, window):
    node = (N - 1, 0, 5)
    pos = np.array([node]) * (np.asarray(L) / N)
    plain = hn.paint(pos, N, L, window)
    assert np.max(np.abs(np.fft.fftn(plain) - pc.spike_spectrum(node, N, window))) < 1e-13
    comp = hn.paint(pos, N, L, window, compensated=True)
    want = pc.compensated_spike_spectrum(node, N, window)
    assert np.max(np.abs(np.fft.fftn(comp) - want)) < 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(want)) > 1.5 and abs(want[0, 0, 0] - 1.) < 1e-15          # not flat; the mean is kept


# ---- 4. COLA ------------------------------------------------------------------------------------------------------------------
def _rel(a, b, scale=None):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) if scale is None else scale))


@pytest.mark.parametrize("N,L", pc.cola_geometries())
def test_lpt_closed_forms(N, L):
    for axis in range(3):
        d = pc.nyquist_wave(N, axis)
        assert abs(d.sum()) == 0. and np.array_equal(np.abs(d), np.full((N, N, N), 0.25))
        p1, p2 = cn.lpt(d, L)
        assert max(np.max(np.abs(p1)), np.max(np.abs(p2))) < 1e-12 * 0.25 * L
    d, w1, w2 = pc.two_waves(N, L)
    assert np.max(np.abs(w2[1])) > 1e-3 * np.max(np.abs(w1[1])) and not w1[0].any() and not w2[2].any()
    for dtype, tol in ((F64, 1e-12), (F32, 3e-6)):
        p1, p2 = cn.lpt(d, L, dtype)
        assert _rel(p1, w1) < tol and _rel(p2, w2) < tol, dtype
    g = pc.gaussian_field(N)
    a, b = cn.lpt(g, L), cn.lpt(g, L, F32)
    assert 1e-8 < _rel(b[0], a[0]) < 3e-6 and 1e-8 < _rel(b[1], a[1]) < 3e-6    # delta_ref of the GPU test: fp32, not fp64


@pytest.mark.parametrize("N,L", pc.cola_geometries())
def test_init_wraps_by_construction(N, L):
    psi1, psi2, want, special = pc.init_displacements(N, L)
    assert _same_in_fp32(psi1) and _same_in_fp32(psi2) and len(special) == 18
    raw = (cn.lagrangian(N, L) + psi1.reshape(3, -1).T) + psi2.reshape(3, -1).T
    assert raw.min() <= -2.5 * L and raw.max() >= 3.25 * L and np.any(raw == L) and np.any((raw < 0) & (raw > -1e-10))
    got = cn.init(psi1, psi2, L, 1., 1.)
    np.testing.assert_array_equal(got, want)
    assert np.all((got >= 0.) & (got < L))
    for p, a, name in special:
        assert got[p, a] == {"to -2.5 L": 0.5 * L, "to +3.25 L": 0.25 * L}.get(name, 0.), name


@pytest.mark.parametrize("N,L", pc.cola_geometries())
def test_kick_readout_by_construction(N, L):
    pos, m, f = pc.kick_particles(N, L)
    assert np.any((m == N - 1) & (f > 0)) and np.any(f == 0)
    zero = np.zeros((3, N, N, N))
    coef = [1., 0., 0., 0., 0., 0.]
    for dtype in (F64, F32):
        pres, p2 = cn.kick(np.full((3, N, N, N), 3.25), zero, zero, zero, pos, L, coef, 0, dtype)
        assert np.all(pres == 3.25) and p2 is pos
        pres, _ = cn.kick(pc.linear_force(N), zero, zero, zero, pos, L, coef, 0, dtype)
        np.testing.assert_array_equal(pres.reshape(3, -1).T, pc.linear_readout(m, f, N))
    last = (m[:, 0] == N - 1) & (f[:, 0] == 0.625)
    assert last.any() and np.all(pc.linear_readout(m, f, N)[last, 0] == 0.375 * 0.5 * (N - 1))
    # drift: with p_res = 0, Dr = 0, dD1 = dD2 = 1 the drift is init's expression from the Lagrangian nodes
    psi1, psi2, want, _ = pc.init_displacements(N, L)
    _, moved = cn.kick(zero, psi1, psi2, zero, cn.lagrangian(N, L), L, [0., 0., 0., 0., 1., 1.], 1)
    np.testing.assert_array_equal(moved, want)


@pytest.mark.parametrize("N,L", pc.cola_geometries())
def test_readout_is_the_transpose_of_paint(N, L):
    rs = np.random.RandomState(N)
    pos = np.concatenate([pc.tiled_positions(N, L)[:N ** 3 // 2], rs.uniform(-L, 2 * L, (N ** 3 - N ** 3 // 2, 3))])
    F = rs.normal(size=(3, N, N, N))
    w = rs.normal(size=N ** 3)
    g = cn.readout(F, pos, N, L)
    mesh = cn.paint(pos, N, L, w)
    aw = cn.paint(pos, N, L, np.abs(w))
    for c in range(3):
        lhs, rhs = math.fsum(w * g[:, c]), math.fsum((F[c] * mesh).reshape(-1))
        assert abs(lhs - rhs) <= 2 * math.fsum(pc.sum_bound(np.abs(F[c]) * aw).reshape(-1)), c
    assert abs(math.fsum(w * g[:, 0])) > 1.


def test_velocity_and_grid_velocity_statements():
    N = 16
    rs = np.random.RandomState(2)
    p1, p2, pr = rs.normal(size=(3, 3, N, N, N))
    v = cn.velocity(p1, p2, pr, 0.5, -0.25, 100.)
    assert v.shape == (N ** 3, 3) and v[5, 1] == 100. * ((pr[1].flat[5] + 0.5 * p1[1].flat[5]) + -0.25 * p2[1].flat[5])
    count = rs.randint(0, 3, (N, N, N)).astype(F64)
    num = rs.normal(size=(N, N, N))
    gv = cn.grid_velocity(num, count, F32)
    assert (count == 0).sum() > 100 and np.all(gv[count == 0] == 0.) and np.all(np.isfinite(gv)) and _same_in_fp32(gv)


def test_stage_chain_is_run():
    N, L, n_steps = 16, 32., 2
    cosmo = Cosmology(Omega_c=0.25, Omega_b=0.05, h=0.7)
    d0 = pc.gaussian_field(N)
    o = cn.run(d0, L, cosmo, 0., 15., n_steps)
    tab = cola.launch_table(cola.Growth(cosmo), 0., 15., n_steps)
    assert tab.size == 3 + 6 * (n_steps + 1)
    psi1, psi2 = cn.lpt(d0, L)
    pos = cn.init(psi1, psi2, L, tab[0], tab[1])
    pres = np.zeros((3, N, N, N))
    for j in range(n_steps + 1):
        count, F = cn.force(pos, N, L, tab[2])
        pres, pos = cn.kick(F, psi1, psi2, pres, pos, L, tab[3 + 6 * j: 9 + 6 * j], j < n_steps)
    np.testing.assert_array_equal(pos, o["pos"])
    np.testing.assert_array_equal(pres.reshape(3, -1).T, o["pres"])
    np.testing.assert_array_equal(count - 1., o["delta"])
