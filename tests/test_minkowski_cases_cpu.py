"""CPU: the numpy statement of the Minkowski-functional counts (tests/minkowski_numpy.py), the constructed cases
(tests/minkowski_cases.py) and the host formulas of fastbox_amd/minkowski.py, validated without a GPU: against a brute-force cell
complex, against literal integers, and against the Gaussian expectations."""
import numpy as np
import pytest

from fastbox_amd import minkowski as mk
from tests import minkowski_cases as mc
from tests import minkowski_numpy as mn

# N = 16, threshold 0.5: n3, n2 (x, y, z), n1 (x, y, z), n0, chi
LITERAL_16 = {
    "one voxel": (1, (2, 2, 2), (4, 4, 4), 8, 1),
    "pair along x": (2, (3, 4, 4), (8, 6, 6), 12, 1),
    "pair along x across the seam": (2, (3, 4, 4), (8, 6, 6), 12, 1),
    "pair sharing an edge": (2, (4, 4, 4), (8, 8, 7), 14, 1),
    "pair sharing a vertex": (2, (4, 4, 4), (8, 8, 8), 15, 1),
    "pair sharing a vertex across the seam": (2, (4, 4, 4), (8, 8, 8), 15, 1),
    "3^3 shell, centre out": (26, (36, 36, 36), (48, 48, 48), 64, 2),
    "3 x 3 ring in a z-plane": (8, (12, 12, 16), (24, 24, 16), 32, 0),
    "full z-plane": (256, (256, 256, 512), (512, 512, 256), 512, 0),
    "rod along x": (16, (16, 32, 32), (64, 32, 32), 64, 0),
    "full box": (4096, (4096,) * 3, (4096,) * 3, 4096, 0),
    "full box minus one voxel": (4095, (4096,) * 3, (4096,) * 3, 4096, 1),
}


def _as_tuple(c, j=0):
    return (int(c["n3"][j]), tuple(int(v) for v in c["n2"][:, j]), tuple(int(v) for v in c["n1"][:, j]), int(c["n0"][j]))


@pytest.mark.parametrize("N", (5, 6, 7))
def test_statement_is_the_brute_force_complex(N):
    """Random binary fields at three fillings: every count of the statement equals the set-built cell complex."""
    rs = np.random.RandomState(N)
    for fill in (0.1, 0.4, 0.8):
        mask = rs.random_sample((N, N, N)) < fill
        c = mn.counts_3d(mask.astype(np.float64), [mc.THRESHOLD])
        b = mc.brute_force_3d(mask)
        assert _as_tuple(c) == (b["n3"], b["n2"], b["n1"], b["n0"])
        m2 = mask[:, :, 0]
        c2, b2 = mn.counts_2d_map(m2.astype(np.float64), [mc.THRESHOLD]), mc.brute_force_2d(m2)
        assert (int(c2["n2"][0]), tuple(int(v) for v in c2["n1"][:, 0]), int(c2["n0"][0])) == (b2["n2"], b2["n1"], b2["n0"])


def test_bodies_have_the_literal_counts_at_16():
    got = {name: (e["n3"], e["n2"], e["n1"], e["n0"], e["chi"]) for name, _, e in mc.bodies(16)}
    assert got == LITERAL_16


@pytest.mark.parametrize("N", (16, 18, 30))
def test_statement_gives_the_constructed_counts(N):
    cases = mc.cases_3d(N)
    assert len(cases) == 3 * len(LITERAL_16)
    for name, field, e in cases:
        c = mn.counts_3d(field, [mc.THRESHOLD])
        assert _as_tuple(c) == (e["n3"], e["n2"], e["n1"], e["n0"]), name
        assert int(mn.euler_3d(c)[0]) == e["chi"], name
    # the rod along x really lies along x in the unpermuted case: an orientation that the permuted cases then move
    rod = [f for n, f, _ in cases if n == "rod along x, axes xyz"][0]
    assert rod[:, 4, 5].sum() == N and rod.sum() == N


@pytest.mark.parametrize("N", (16, 18))
def test_statement_gives_the_constructed_counts_per_channel(N):
    for name, m, e in mc.shapes_2d(N):
        c = mn.counts_2d_map(m, [mc.THRESHOLD])
        assert (int(c["n2"][0]), tuple(int(v) for v in c["n1"][:, 0]), int(c["n0"][0])) == (e["n2"], e["n1"], e["n0"]), name
        assert int(mn.euler_2d(c)[0]) == e["chi"], name
    cube, e = mc.channel_cube(N)
    c = mn.counts_per_channel(cube, [mc.THRESHOLD])
    np.testing.assert_array_equal(c["n2"][:, 0], e["n2"])
    np.testing.assert_array_equal(c["n1"][:, :, 0], e["n1"])
    np.testing.assert_array_equal(c["n0"][:, 0], e["n0"])
    np.testing.assert_array_equal(mn.euler_2d(c)[:, 0], e["chi"])


def test_statement_thresholds_nan_and_infinities():
    f = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    f[0, 0, 0], f[1, 1, 1], f[2, 2, 2] = np.nan, np.inf, -np.inf
    c = mn.counts_3d(f, [-1e300, 5., 5.5, 1e300])
    assert c["n_nan"] == 1 and list(c["n3"]) == [25, 21, 20, 1]            # 5 >= 5 counts; +inf is above 1e300
    assert list(c["n0"]) == [27, 27, 27, 8]                                 # a vertex touches 8 voxels; 8 vertices touch the inf one


def test_formulas_on_a_cuboid():
    """One voxel in a cuboid box: surface 2 (ab + bc + ca), mean-breadth sum a + b + c, chi = 1, by hand."""
    N, L = 16, (32., 48., 80.)
    a, b, c = [s / N for s in L]
    V = L[0] * L[1] * L[2]
    v0, v1, v2, v3 = mk.minkowski_from_counts([1], [[2], [2], [2]], [[4], [4], [4]], [8], N, L)
    assert v0[0] == 1. / N ** 3 and v3[0] == pytest.approx(1. / V, rel=1e-15)
    assert v1[0] == pytest.approx(2. * (b * c + a * c + a * b) / (9. * V), rel=1e-14)
    assert v2[0] == pytest.approx(2. * (a + b + c) / (9. * V), rel=1e-14)
    # a cube: the closed forms 2 (n2 - 3 n3) / (9 a N^3) and 2 (n1 - 2 n2 + 3 n3) / (9 a^2 N^3) with the summed counts
    n3, n2, n1, n0 = 26., 108., 144., 64.
    w = mk.minkowski_from_counts([n3], [[36]] * 3, [[48]] * 3, [n0], N, 32.)
    assert w[1][0] == pytest.approx(2. * (n2 - 3 * n3) / (9. * 2. * N ** 3), rel=1e-14)
    assert w[2][0] == pytest.approx(2. * (n1 - 2 * n2 + 3 * n3) / (9. * 4. * N ** 3), rel=1e-14)
    assert w[3][0] == pytest.approx(2. / 32. ** 3, rel=1e-14)
    u0, u1, u2 = mk.minkowski_from_counts_2d([1], [[2], [2]], [4], N, (32., 48.))
    assert u0[0] == 1. / N ** 2 and u2[0] == pytest.approx(1. / (32. * 48.), rel=1e-15)
    assert u1[0] == pytest.approx(np.pi * (2. * a + 2. * b) / (16. * 32. * 48.), rel=1e-14)


def _deviation(measured, theory):
    return [float(np.max(np.abs(m - t)) / np.max(np.abs(t))) for m, t in zip(measured, theory)]


def test_gaussian_theory_3d():
    """64^3, R = 2 voxels, seeds 0 .. 3, nu = linspace(-3, 3, 25): the mean measured functionals against Tomita's expectations.
    Measured with the statement: 0.001, 0.013, 0.047, 0.045 of max|theory| for V0 .. V3; bounds 0.005, 0.03, 0.10, 0.10."""
    N, nu = 64, np.linspace(-3., 3., 25)
    meas, theo = [], []
    for seed in range(4):
        f, ratio = mc.gaussian_field(N, 2., seed)
        c = mn.counts_3d(f, nu)
        meas.append(mk.minkowski_from_counts(c["n3"], c["n2"], c["n1"], c["n0"], N, float(N)))
        theo.append(mk.gaussian_minkowski(nu, 1., ratio, dim=3))
    dev = _deviation(np.mean(meas, axis=0), np.mean(theo, axis=0))
    print("3-D deviations V0 .. V3:", ["%.4f" % d for d in dev])
    assert all(d <= b for d, b in zip(dev, (0.005, 0.03, 0.10, 0.10))), dev


def test_gaussian_theory_2d():
    """256^2, R = 2 pixels, seeds 0 .. 7: measured 0.005, 0.015, 0.042 of max|theory| for v0, v1, v2; bounds 0.02, 0.05, 0.10."""
    N, nu = 256, np.linspace(-3., 3., 25)
    meas, theo = [], []
    for seed in range(8):
        f, ratio = mc.gaussian_field(N, 2., seed, dim=2)
        c = mn.counts_2d_map(f, nu)
        meas.append(mk.minkowski_from_counts_2d(c["n2"], c["n1"], c["n0"], N, float(N)))
        theo.append(mk.gaussian_minkowski(nu, 1., ratio, dim=2))
    dev = _deviation(np.mean(meas, axis=0), np.mean(theo, axis=0))
    print("2-D deviations v0 .. v2:", ["%.4f" % d for d in dev])
    assert all(d <= b for d, b in zip(dev, (0.02, 0.05, 0.10))), dev
