"""The constructed catalogues of the three-point tests (tests/test_threepoint_cases_cpu.py asserts on the CPU what each is for;
tests/test_threepoint_gpu.py runs them on the device).  ``all_cases()`` builds them once, ``reference(i)`` and
``legendre(i)`` hold the two numpy statements of tests/threepoint_numpy.py for case i, computed once and shared."""
import functools

import numpy as np

from fastbox_amd import rng
from tests import threepoint_numpy as tn

COS_THETA = -0.3                         # the triangle's opening angle at particle 0
CROWD = (63, 64, 65, 255, 256, 257, 511, 512, 513)   # in-range neighbours of the chosen primaries of the crowded case: round
                                                      # the tile of 64, a stride of 256 and the sweep's stride of 512
DR_SEED, DR_PER_DATUM = 11, 4

NAMES = ("1 triangle", "2 seam", "3 two cells per axis", "4 lattice on edges", "5 crowded", "6 coincident", "7 lonely primary",
         "8 cuboid mixed-sign weights", "9 minimal", "10 D - R", "11 crowded, lmax = 8")


def _case(name, L, pos, edges, lmax, weights=None, probe=(), **extra):
    L = (float(L),) * 3 if np.ndim(L) == 0 else tuple(float(a) for a in L)
    c = dict(name=name, L=L, pos=np.ascontiguousarray(pos, dtype=np.float64), edges=np.asarray(edges, dtype=np.float64),
             lmax=int(lmax), weights=None if weights is None else np.asarray(weights, dtype=np.float64),
             probe=np.asarray(probe, dtype=np.int64))
    c.update(extra)
    return c


def _shell_points(rs, k, rmin, rmax):
    """k offsets in random directions with lengths uniform in [rmin, rmax]."""
    v = rs.standard_normal((k, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return v * rs.uniform(rmin, rmax, k)[:, None]


@functools.lru_cache(maxsize=None)
def all_cases():
    rs = np.random.RandomState(2015)
    cases = []
    # 1. three particles: 0-1 at 1.5 (bin 0), 0-2 at 2.5 (bin 1), 1-2 beyond the last edge
    u1, v = np.array([1., 2., 2.]) / 3., np.array([2., 1., -2.]) / 3.
    u2 = COS_THETA * u1 + np.sqrt(1. - COS_THETA ** 2) * v
    p0 = np.array([5., 6., 7.])
    cases.append(_case(NAMES[0], 20., [p0, p0 + 1.5 * u1, p0 + 2.5 * u2], [1., 2., 3.], 10, probe=(0, 1, 2)))
    # 2. the same cluster, offsets in 64ths so that every difference is exact, inside one cell and across the corner
    off = rs.randint(-96, 97, (14, 3)) / 64.
    cases.append(_case(NAMES[1], 20., np.concatenate([7.5 + off, off]), [0.5, 1.5, 3.], 8, probe=(0, 5, 14, 19), half=14))
    # 3. L = 10, last edge 4.9: two cells per axis
    cases.append(_case(NAMES[2], 10., rs.uniform(0., 10., (150, 3)), [1., 2.5, 4.9], 6, probe=(0, 77, 149)))
    # 4. the unit lattice: d^2 = 1 and 4 fall on edges
    g = np.arange(6.)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    cases.append(_case(NAMES[3], 6., lattice, [1., 1.5, 2., 2.5], 5, probe=(0, 100, 215)))
    # 5. isolated clusters: primary k has exactly CROWD[k] neighbours in range; then one cell of the sweep with 1100 particles
    pts, centres = [], []
    for k, m in enumerate(CROWD):
        c = np.array([6. + 12. * (k % 3), 6. + 12. * (k // 3), 6.])
        centres.append(len(pts))
        pts.append(c)
        pts.extend(c + _shell_points(rs, m, 0.3, 0.95))
    pts.extend(rs.uniform(33.4, 36.6, (1100, 3)))
    cases.append(_case(NAMES[4], 40., np.array(pts), [0.25, 0.5, 1.], 4, probe=centres + [len(pts) - 1], centres=centres,
                       cells=(12, 12, 12), crowded_cell=(10, 10, 10)))
    # 6. duplicated points: each is skipped for its twin (d^2 = 0 < e_0^2) but counted for third parties
    base = rs.uniform(0., 10., (40, 3))
    cases.append(_case(NAMES[5], 10., np.concatenate([base, base[:10]]), [0.5, 1.5, 3.], 5, probe=(0, 40, 9, 49, 20)))
    # 7. a cluster and one primary with no neighbour
    cases.append(_case(NAMES[6], 20., np.concatenate([5. + _shell_points(rs, 20, 0., 1.5), [[15., 15., 15.]]]), [0.5, 1.5, 3.], 3,
                       probe=(20, 0)))
    # 8. a cuboid, weights of both signs, the largest table: lmax = 10, nr = 20
    cases.append(_case(NAMES[7], (8., 10., 12.), rs.uniform(-5., 15., (400, 3)), np.linspace(0.4, 3.9, 21), 10,
                       weights=rs.standard_normal(400), probe=(0, 1, 399)))
    # 9. lmax = 0, nr = 1
    cases.append(_case(NAMES[8], 10., rs.uniform(0., 10., (100, 3)), [1., 3.], 0, probe=(0, 99)))
    # 10. 300 clustered data and 1200 randoms (the host model of uniform_catalogue) with weight -W_d / n_r: N = D - R
    data = wrap_into(np.concatenate([c + 1.2 * rs.standard_normal((50, 3)) for c in rs.uniform(0., 20., (6, 3))]), 20.)
    rand = rng.recon_uniforms(DR_PER_DATUM * 300, (20., 20., 20.), DR_SEED, 0)
    cases.append(_case(NAMES[9], 20., np.concatenate([data, rand]), [1., 2., 3., 4.], 4,
                       weights=np.concatenate([np.ones(300), np.full(1200, -300. / 1200.)]), probe=(0, 299, 300, 1499), n_data=300))
    # 11. the crowded catalogue again with a table of more than 64 rows: the sweep's workgroup of 512 and its strides
    cases.append(dict(cases[4], name=NAMES[10], lmax=8))
    assert tuple(c["name"] for c in cases) == NAMES
    return tuple(cases)


def wrap_into(x, L):
    return x - L * np.floor(x / L)


def index_of(name):
    return NAMES.index(name)


@functools.lru_cache(maxsize=None)
def reference(index):
    c = all_cases()[index]
    return tn.alm_statement(c["pos"], c["weights"], c["L"], c["edges"], c["lmax"])


@functools.lru_cache(maxsize=None)
def legendre(index):
    c = all_cases()[index]
    return tn.legendre_statement(c["pos"], c["weights"], c["L"], c["edges"], c["lmax"])


@functools.lru_cache(maxsize=None)
def largest_gap():
    """g: the largest gap between the two statements over the cases, in units of T."""
    return max(tn.gap(reference(i), legendre(i)) for i in range(len(NAMES)))
