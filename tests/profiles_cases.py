"""The constructed halo-profile cases: tests/test_profiles_cases_cpu.py asserts on the CPU the property that keeps each one
from being vacuous, tests/test_profiles_gpu.py runs them on the device.  A case is a dict: name, L (3,), pos (n, 3), centres
(nh, 3), edges, and where it applies vel (n, 3), r2 (nh,) -- the squared aperture radii -- expect_inner / expect_counts (rows
stated by hand) and so (keywords of the spherical-overdensity finish).  Coordinates are dyadic wherever an equality is meant
to be exact."""
import functools

import numpy as np

from tests import profiles_numpy as pf
from tests.fof_numpy import wrap


def _case(name, L, pos, centres, edges, **extra):
    L = (float(L),) * 3 if np.isscalar(L) else tuple(float(a) for a in L)
    d = dict(name=name, L=L, pos=np.ascontiguousarray(pos, dtype=np.float64), centres=np.ascontiguousarray(centres, dtype=np.float64),
             edges=np.asarray(edges, dtype=np.float64), vel=None, r2=None, so=None, expect_inner=None, expect_counts=None)
    d.update(extra)
    return d


def _uniform(L, n, seed):
    return np.random.RandomState(seed).uniform(0., 1., (n, 3)) * np.asarray(L, dtype=np.float64)


# ---- 1: particles exactly on edges, and on the centre --------------------------------------------------------------------
EDGE_OFFSETS = np.array([[0., 0., 0.],            # on the centre: d^2 = 0
                         [0.25, 0., 0.],          # inside e0 = 0.5
                         [0.5, 0., 0.],           # d^2 = e0^2: bin 0
                         [0., -1., 0.],           # inside bin 0
                         [0.75, 1., 0.],          # 3-4-5: d^2 = 1.5625 = 1.25^2, the interior edge: bin 1
                         [0., 0., 1.5],           # inside bin 1
                         [0., 0., -2.],           # d^2 = the last edge squared: excluded
                         [2., 2., 2.]])           # beyond


def case_edges(e0):
    """One centre at (4, 4, 4) of L = 16 and eight particles at dyadic offsets; edges (e0, 1.25, 2) with e0 = 0.5, or
    (0, 0.5, 1.25, 2): the particle on the centre is in ``inner`` with e0 > 0 and in bin 0 with e0 = 0."""
    c = np.array([[4., 4., 4.]])
    if e0 > 0.:
        return _case("1 edges e0=0.5", 16., c + EDGE_OFFSETS, c, [0.5, 1.25, 2.], expect_inner=[2], expect_counts=[[2, 2]])
    return _case("1 edges e0=0", 16., c + EDGE_OFFSETS, c, [0., 0.5, 1.25, 2.], expect_inner=[0], expect_counts=[[2, 2, 2]])


# ---- 2: a centre at the corner of the box, neighbours across all three faces -----------------------------------------------
SEAM_C = np.array([2. ** -40, 8. - 2. ** -40, 2. ** -40])


def case_seam():
    """L = 8.  Centre 0 is within 2^-40 of the corner (0, 8, 0); centre 1 is the same point given as c + (L, -2L, 3L) (exact
    in fp64: the rows must be identical); centre 2 is the largest double below L on every axis.  400 particles fill the cube of
    side 4 around the corner, in all eight octants, and 100 the rest of the box."""
    rs = np.random.RandomState(21)
    pos = np.concatenate([wrap(rs.uniform(-2., 2., (400, 3)), np.array([8., 8., 8.])), rs.uniform(0., 8., (100, 3))])
    top = np.nextafter(8., 0.)
    centres = np.stack([SEAM_C, SEAM_C + np.array([8., -16., 24.]), np.array([top, top, top])])
    return _case("2 seam", 8., pos, centres, np.linspace(0.25, 1.75, 7))


# ---- 3: a cuboid box with 2, 3 and 7 cells along the axes ------------------------------------------------------------------
CUBOID_L, CUBOID_CELLS = (8., 12., 40.), (2, 3, 7)


def case_cuboid():
    """700 particles, so that the cell grid of reach 3.9 is (2, 3, 7): along x the offsets -1 and +1 name one cell, along y
    all three cells are neighbours, along z the column crosses the seam for the centres of the first and last cell."""
    pos = _uniform(CUBOID_L, 700, 31)
    centres = np.concatenate([_uniform(CUBOID_L, 60, 32), [[0., 0., 0.], [7.9, 11.9, 39.9], [4., 6., 0.5], [4., 6., 39.5]]])
    return _case("3 cuboid (2, 3, 7) cells", CUBOID_L, pos, centres, np.linspace(0., 3.9, 7))


# ---- 4: one crowded cell, the thread-stride boundaries ---------------------------------------------------------------------
CROWDED = (255, 256, 257, 1025)


def case_crowded(k):
    """L = 32: k particles inside [13.1, 14.9]^3, which lies inside one cell for the 4, 5 or 8 cells per axis these sizes
    get; every other cell is empty.  Centres inside the blob, and one 3.5 along x from its middle: in the next cell where the
    cells are 4 or 8 wide."""
    pos = 13.1 + 1.8 * np.random.RandomState(40 + k % 7).uniform(0., 1., (k, 3))
    centres = np.array([[14., 14., 14.], [13.5, 14.5, 14.25], [17.5, 14., 14.]])
    return _case("4 crowded cell of %d" % k, 32., pos, centres, [0., 0.5, 1., 2., 3.9])


# ---- 5: more centres than workgroups ---------------------------------------------------------------------------------------
def case_many():
    """3000 centres over 5000 particles: more centres than the sweep has workgroups (8 per compute unit: 2048 on 256 units),
    so that the grid-stride loop runs; centres 0 and 1 are identical."""
    centres = _uniform((32.,) * 3, 3000, 52)
    centres[1] = centres[0]
    return _case("5 many centres", 32., _uniform((32.,) * 3, 5000, 51), centres, np.linspace(0.5, 3., 6))


# ---- 6: the least and the most bins ----------------------------------------------------------------------------------------
def case_bins(nr):
    edges = [1., 3.] if nr == 1 else np.linspace(0., 3.5, nr + 1)
    return _case("6 nr=%d" % nr, 16., _uniform((16.,) * 3, 800, 61), _uniform((16.,) * 3, 20, 62), edges)


# ---- 7: blobs on a uniform background --------------------------------------------------------------------------------------
BLOB_CENTRES = np.array([[10., 12., 20.], [22., 7., 9.], [31.9, 0.2, 31.7]])       # the last one across a corner
BLOB_N, BLOB_SIGMA = (600, 150, 1200), (0.5, 0.3, 0.8)


def blob_positions():
    rs = np.random.RandomState(71)
    parts = [rs.uniform(0., 32., (4096, 3))]
    for c, n, s in zip(BLOB_CENTRES, BLOB_N, BLOB_SIGMA):
        parts.append(wrap(c + s * rs.standard_normal((n, 3)), np.array([32., 32., 32.])))
    return np.concatenate(parts)


def void_centre(pos, L=32., step=2.):
    """The node of a coarse lattice that is farthest from every particle."""
    from scipy.spatial import cKDTree
    k = np.arange(0.5 * step, L, step)
    g = np.stack(np.meshgrid(k, k, k, indexing='ij'), axis=-1).reshape(-1, 3)
    d, _ = cKDTree(pos, boxsize=L).query(g)
    return g[np.argmax(d)], float(d.max())


def case_blobs(rmax):
    """L = 32, 4096 uniform points and three Gaussian blobs; 24 logarithmic bins from 0.05 to ``rmax``.  Unit particle mass
    and rho_ref = the mean number density: with rmax = 4 the three blobs have status 0 at Delta = 200 and 500 and the fourth
    centre, in a void, has status 1; with rmax = 0.3 the blobs are still above both thresholds at the last edge: status 2."""
    pos = blob_positions()
    centres = np.concatenate([BLOB_CENTRES, void_centre(pos)[0][None, :]])
    so = dict(particle_mass=1., rho_ref=pos.shape[0] / 32. ** 3, deltas=(200., 500.))
    return _case("7 blobs rmax=%g" % rmax, 32., pos, centres, np.geomspace(0.05, rmax, 25), so=so)


# ---- 8: apertures ------------------------------------------------------------------------------------------------------------
def case_apertures():
    """L = 16, 600 uniform particles and five placed by hand; centres at dyadic points with their own radii: centre 0 has
    R^2 = 0 (a particle sits on it: not a member, m = 0); centre 1 has a particle at d^2 = R^2 = 1.5625 exactly (excluded)
    and one just inside; centres 2-4 have R = 1.9, 2.5 and 3.9, centre 4 at the corner of the box.  Velocities: a common
    flow of (3000, -2000, 1000) km/s and a scatter of 5 km/s, so that sigma_v is a small difference of large numbers."""
    rs = np.random.RandomState(81)
    centres = np.array([[4., 4., 4.], [8., 8., 8.], [12., 4., 10.], [5., 11., 3.], [0., 16., 0.]])
    placed = np.array([[4., 4., 4.], [8.75, 9., 8.], [8.5, 8., 8.5], [8., 8., 8.], [15.5, 0.25, 15.75]])
    pos = np.concatenate([rs.uniform(0., 16., (600, 3)), placed])
    vel = np.array([3000., -2000., 1000.]) + 5. * rs.standard_normal(pos.shape)
    r2 = np.array([0., 1.5625, 1.9 ** 2, 2.5 ** 2, 3.9 ** 2])
    return _case("8 apertures", 16., pos, centres, [0.5, 3.9], vel=vel, r2=r2)


def all_cases():
    return ([case_edges(0.5), case_edges(0.), case_seam(), case_cuboid()] + [case_crowded(k) for k in CROWDED]
            + [case_many(), case_bins(1), case_bins(256), case_blobs(4.), case_blobs(0.3), case_apertures()])


NAMES = [c["name"] for c in all_cases()]


def index_of(name):
    return NAMES.index(name)


@functools.lru_cache(maxsize=None)
def reference(index):
    """(case, inner, counts) of all_cases()[index] by the numpy statement, computed once and shared; arrays are read-only."""
    case = all_cases()[index]
    inner, counts = pf.profiles(case["centres"], case["pos"], case["L"], case["edges"])
    for a in (case["pos"], case["centres"], case["edges"], case["vel"], case["r2"], inner, counts):
        if a is not None:
            a.setflags(write=False)
    return case, inner, counts


@functools.lru_cache(maxsize=None)
def aperture_reference(index):
    case = all_cases()[index]
    return pf.apertures(case["centres"], case["pos"], case["L"], case["r2"], case["vel"])
