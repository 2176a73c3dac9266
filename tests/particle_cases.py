"""Constructed inputs for the particle-mesh kernels (fb_halo.hip, fb_cola.hip), numpy only: the cases that a realised Gaussian
density never produces -- expected counts from 1e-300 to 2^24, integer expectations, one voxel past the limit; counts that
take every path of the catalogue's tables; particles on nodes, on cell midpoints and on the seam of the box; displacements of
several box lengths.  Positions are dyadic fractions of a cell whose size is a power of two and weights are small integers or
powers of two, so every expected value below is exact in fp64 (and in fp32 where it fits 24 bits) and is written down from the
definition -- the window W(s) at the distance s between node and particle, in rational arithmetic -- not from a second copy of
the kernels' floor / fraction formulas.  tests/test_particle_cases_cpu.py holds the numpy statements (tests/halos_numpy.py,
tests/cola_numpy.py, fastbox_amd/rng.py) to these cases and asserts the property that keeps each from being vacuous;
tests/test_particle_edges_gpu.py runs them on the device."""
from fractions import Fraction

import numpy as np

from tests import halos_numpy as _hn

LAM_MAX = 2. ** 24
WINDOWS = ("ngp", "cic", "tsc")


# ---- 1. expected counts over the whole range ----------------------------------------------------------------------------------
def lambda_classes(N):
    """One expected count per z index: 1e-300, 1e-3, 0.5, 1, 2, 3, then log-spaced from 10 to 2^24 / 1.1."""
    return np.concatenate([[1e-300, 1e-3, 0.5, 1., 2., 3.], np.geomspace(10., LAM_MAX / 1.1, N - 6)])


def poisson_box(N):
    """dict(L, delta, nbar, bias, classes, int_row, top): a box of unit voxels (L = N) with bias 1, so that the expected count is
    the single product nbar (1 + delta).  nbar is the class value of the voxel's z index; delta is a multiple of 2^-10 within
    +-102/1024 (the same number in fp32 and fp64, and 1 + delta is exact), which spreads each class by +-10 %.  In the row
    int_row = (ix, iy) delta is 0 and nbar the class value rounded to an integer >= 1: an integer expected count, the mode on
    lam itself.  At the voxel ``top`` nbar = 2^24 and delta = 0: the largest count that is drawn."""
    cls = lambda_classes(N)
    rs = np.random.RandomState(1234 + N)
    delta = rs.randint(-102, 103, (N, N, N)) / 1024.
    nbar = np.broadcast_to(cls, (N, N, N)).copy()
    int_row = (3, 5)
    delta[int_row] = 0.
    nbar[int_row] = np.maximum(1., np.rint(cls))
    top = (N - 2, 1, N - 1)
    delta[top], nbar[top] = 0., LAM_MAX
    return dict(L=(float(N),) * 3, delta=delta, nbar=nbar, bias=1., classes=cls, int_row=int_row, top=top)


def poisson_unit(lam):
    """The unit of the bracket: 2^-52 max(floor(lam) ln lam, 1).  The log-pmf at the mode, (m ln lam - lam) - lgamma(m + 1), is
    three roundings of numbers no larger than m ln lam, plus a few ulp of log and lgamma, whose results are no larger either;
    the pmf at the mode, and with it the whole CDF the walk builds on it, carries that as a relative error."""
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(lam >= 1., np.floor(lam) * np.log(lam), 0.)
    return 2. ** -52 * np.maximum(t, 1.)


def poisson_bracket(k, lam, u):
    """(slack, n_ppf): the largest slack, in units, that cdf(k - 1) - s <= u < cdf(k) + s needs over all voxels (0: none), and
    the number of voxels where k is not scipy's poisson.ppf(u, lam)."""
    from scipy.stats import poisson
    k, lam, u = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (k, lam, u)]
    need = np.maximum(poisson.cdf(k - 1., lam) - u, u - poisson.cdf(k, lam))
    slack = float(np.max(np.maximum(need, 0.) / poisson_unit(lam)))
    return slack, int(np.sum(k != poisson.ppf(u, lam)))


def overflow_boxes(N):
    """[(name, voxel, nbar field, delta field)]: poisson_box with delta = 0 at one voxel and nbar there 2^24 + 16 -- an expected
    count of exactly 2^24 (1 + 2^-20), the smallest step above the limit that fp32 would still see -- or +inf: in turn the last
    voxel of the grid and a voxel that is lane 37 of its wave (flat index 5 * 256 + 37).  With nbar = 2^24 at the same
    voxel the expected count is the limit itself, which must draw."""
    b = poisson_box(N)
    out = []
    for value, tag in ((LAM_MAX + 16., "above"), (np.inf, "inf")):
        for flat in (N ** 3 - 1, 5 * 256 + 37):
            nb, d = b["nbar"].copy(), b["delta"].copy()
            vox = np.unravel_index(flat, nb.shape)
            nb[vox], d[vox] = value, 0.
            out.append(("%s at %d" % (tag, flat), vox, nb, d))
    return out


ODD_DRAW = (7, 0)                  # (seed, realisation) at which the lam = 2^24 voxel of poisson_box(32) draws 2^24 + 811


def lognormal_box(N):
    """(delta, bias): bias * delta covers [-30, 30] in steps of 1/8 (delta a multiple of 1/16, bias 2: the same in fp32), each
    value on many voxels in a seeded order; the extremes are both present."""
    rs = np.random.RandomState(77)
    delta = rs.randint(-240, 241, (N, N, N)) / 16.
    delta[0, 0, 0], delta[N - 1, N - 1, N - 1] = 15., -15.
    return delta, 2.


def lognormal_statements(delta, bias, L, nbar=1.):
    """(the fp64 statement, the same with the maximum of bias delta subtracted before the exponential)."""
    ref = _hn.expected_counts(delta, nbar, bias, L, lognormal=True)
    dh = bias * delta
    e = np.exp(dh - dh.max())
    N = delta.shape[0]
    shifted = (L[0] * L[1] * L[2] / N ** 3. * nbar) * (1. + (e / np.mean(e) - 1.))
    return ref, shifted


def lognormal_deviation(a, ref, scale):
    """Largest |a - ref| over (|ref| + 2 scale): lam = scale (1 + (x - 1)) carries the roundings of two sums of magnitude 1."""
    return float(np.max(np.abs(a - ref) / (np.abs(ref) + 2. * scale)))


def field_params(N):
    """(delta, nbar, bias) fields that differ in every voxel along every axis, all dyadic with few bits: an index error in the
    kernel's parameter fetch changes the product.  nbar in [1, 2), bias in [0.5, 1.5), delta in (-0.5, 0.5)."""
    i = np.arange(N)
    ix, iy, iz = i[:, None, None], i[None, :, None], i[None, None, :]
    nbar = 1. + ((7 * ix + 3 * iy + iz) % 64) / 64.
    bias = 0.5 + ((ix + 5 * iy + 11 * iz) % 32) / 32.
    delta = (((3 * ix + 13 * iy + 5 * iz) % 63) - 31) / 64.
    return delta, nbar, bias


# ---- 2. counts for the catalogue's table paths ------------------------------------------------------------------------------
TILE_MIN, TABLE_MAX, SCAN_CHUNK, LDS_COUNTS = 4096, 2 ** 25, 4096, 4096


def table_layout(n, kmax):
    """(tile, tiles, chunks) of cat_emit in fb_halo.hip, read from its code: the tile starts at 4096 voxels and doubles while
    ceil(n / tile) (kmax + 1) > 2^25 and tile < n; the scan works on chunks of 4096 (count, tile) entries and its top level on
    256 chunks per turn of its carry loop."""
    tile = TILE_MIN
    while -(-n // tile) * (kmax + 1) > TABLE_MAX and tile < n:
        tile *= 2
    tiles = -(-n // tile)
    return tile, tiles, -(-(kmax + 1) * tiles // SCAN_CHUNK)


def catalogue_counts(name, N=64):
    """Poisson(0.7) counts plus constructed voxels.  'atomic': 4095, 4096 and 5000 in different tiles (a tile is one x plane at
    64^3), two voxels of 5000 and two of 4096 inside one 256-voxel step of one tile, and the last voxel of the grid.  'carry': one
    voxel of 20000.  'doubling': one voxel of 600001, next to the boundary between the tiles 2 j + 1 and 2 j + 2 that stays
    and the boundary between 2 j and 2 j + 1 that goes."""
    c = np.random.RandomState(8).poisson(0.7, (N, N, N)).astype(np.int64)
    if name == "atomic":
        c[0, 0, 1], c[3, 4, 5], c[7, 0, 0], c[20, 63, 63] = 4095, 5000, 4096, 4097
        c[41, 2, 3], c[41, 2, 60], c[41, 3, 1], c[41, 3, 2] = 5000, 5000, 4096, 4096      # one step: flat % 4096 in [128, 256)
        c[41, 40, 7] = 5000                                                                # the same tile, a later step
        c[N - 1, N - 1, N - 1] = 5000
    elif name == "carry":
        c[10, 20, 30] = 20000
    elif name == "doubling":
        c[5, 63, 63] = 600001
    else:
        raise ValueError(name)
    return c


# ---- 3. painting ------------------------------------------------------------------------------------------------------------
def window(name, s):
    """The assignment window at the signed distance s = node - particle, in cells (a Fraction).  NGP: the cell (-1/2, 1/2]
    around the particle, so a particle on a midpoint belongs to the upper node.  CIC: 1 - |s|.  TSC: 3/4 - s^2 within 1/2,
    (3/2 - |s|)^2 / 2 out to 3/2."""
    a = abs(s)
    if name == "ngp":
        return Fraction(1) if Fraction(-1, 2) < s <= Fraction(1, 2) else Fraction(0)
    if name == "cic":
        return max(Fraction(0), 1 - a)
    if a <= Fraction(1, 2):
        return Fraction(3, 4) - s * s
    return (Fraction(3, 2) - a) ** 2 / 2 if a < Fraction(3, 2) else Fraction(0)


def expected_mesh(pos, N, L, name, weights=None, return_exact=False, count=False):
    """The mesh of the definition, sum_p w_p prod_a W(node_a - u_a) over the periodic images, in rational arithmetic from the
    positions' exact values; returned as fp64, each node rounded once.  ``return_exact``: also whether no node was rounded (the
    sums fit 53 bits, as in every dyadic case but TSC with weights of 1 beside 2^40).  Particles with a position that is not
    finite are absent.  ``count``: the number of non-zero shares each node receives instead."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    mesh = {}
    for p in range(pos.shape[0]):
        if not np.all(np.isfinite(pos[p])):
            continue
        w = Fraction(1) if weights is None else Fraction(float(weights[p]))
        axes = []
        for a in range(3):
            u = Fraction(float(pos[p, a])) * N / Fraction(float(L[a]))
            base = u.numerator // u.denominator                     # floor
            axes.append([((base + o) % N, window(name, Fraction(base + o) - u)) for o in (-1, 0, 1, 2)])
        for m0, w0 in axes[0]:
            for m1, w1 in axes[1]:
                for m2, w2 in axes[2]:
                    if w0 and w1 and w2:
                        mesh[(m0, m1, m2)] = mesh.get((m0, m1, m2), Fraction(0)) + (1 if count else w * w0 * w1 * w2)
    out = np.zeros((N, N, N))
    exact = True
    for key, v in mesh.items():
        out[key] = float(v)
        exact = exact and Fraction(out[key]) == v
    return (out, exact) if return_exact else out


def paint_geometries():
    """[(N, L)]: a cubic box with cells of 2 and a generic grid (N = 20) whose cells are 1/2, 2 and 8 along x, y and z."""
    return [(16, (32., 32., 32.)), (20, (10., 40., 160.))]


SEAM = ("x = 0", "x = L", "x = L - cell/2", "x = -cell/2", "x = -0.0", "x = 3L + cell/4", "x = -3 cell/4")


def seam_values(N):
    """The seam positions in cells, in the order of SEAM.  (-2^-60 cell is below_zero_positions: its weights are not dyadic.)"""
    return [0., float(N), N - 0.5, -0.5, -0.0, 3. * N + 0.25, -0.75]


def paint_positions(N, L):
    """(pos, labels): a particle on a node, on a cell midpoint, on a midpoint along one axis only, at a quarter; then, for each
    axis in turn, each seam value on that axis with a node and a midpoint on the other two."""
    cell = np.asarray(L) / N
    u = [[3., 5., 7.], [4.5, 9.5, 2.5], [6.5, 2., 11.], [1.25, 8.75, 12.5]]
    labels = ["node", "midpoint", "midpoint on x", "quarter"]
    for a in range(3):
        for name, s in zip(SEAM, seam_values(N)):
            row = [2. + a, 9.5 - a, 13.]
            row[a] = s
            u.append(row)
            labels.append("%s on axis %d" % (name, a))
    return np.array(u) * cell, labels


def below_zero_positions(N, L):
    """One particle per axis at -2^-60 cell on that axis (nodes elsewhere), and the particles at +0 they round to: the fraction
    1 - 2^-60 is 1 in fp64, so all of the mass is on node 0 and none on node N - 1, to 2^-60."""
    cell = np.asarray(L) / N
    u = np.array([[3., 5., 7.]] * 3)
    at0 = u.copy()
    for a in range(3):
        u[a, a], at0[a, a] = -2. ** -60, 0.
    return u * cell, at0 * cell


def dyadic_cloud(N, L, n, seed, ties=True):
    """n particles at multiples of an eighth of a cell over [-N, 2 N) cells; ``ties=False`` leaves out the cell midpoints."""
    rs = np.random.RandomState(seed)
    e = rs.randint(-8 * N, 16 * N, (n, 3))
    if not ties:
        e = np.where(e % 8 == 4, e + 1, e)
    return e / 8. * (np.asarray(L) / N)


def weight_sets(n, seed=5):
    """{name: (weights or None, exact total)}: unweighted; signed small integers; signed integers that sum to exactly 0; weights
    of 1 and 2^40 (five of the latter)."""
    rs = np.random.RandomState(seed)
    signed = rs.randint(-7, 8, n).astype(np.float64)
    zero = signed.copy()
    zero[-1] -= zero.sum()
    span = np.ones(n)
    span[:5] = 2. ** 40
    return {"unweighted": (None, float(n)), "signed": (signed, float(signed.sum())), "zero sum": (zero, 0.),
            "span 2^40": (span, 5 * 2. ** 40 + (n - 5))}


def paint_exponent(weights, n):
    """F of fb_paint's fixed point, from DESIGN.md: contributions are added as round(x 2^F) with F = 61 - e, sum |w| < 2^e (fp32
    plans; fp64 plans carry 32 more bits).  Weights of 1 beside 2^40: e = 43 for five of the latter, F = 18, so a weight-1
    particle's share of a node is kept to 2^-19 absolute on an fp32 plan -- shares below that vanish -- and to 2^-51 on an fp64
    plan, where every dyadic share of these cases is exact."""
    s = float(n) if weights is None else float(np.sum(np.abs(weights)))
    e = int(np.frexp(s)[1]) if s > 0 else 0
    return 61 - e


def reflect_mesh(mesh):
    """node m -> (N - m) % N on every axis."""
    return np.roll(mesh[::-1, ::-1, ::-1], 1, axis=(0, 1, 2))


def spike_spectrum(node, N, name):
    """The DFT of the painted mesh of a unit particle on ``node``, in closed form: exp(-2 pi i m.node / N) for NGP and CIC (all of
    the mass on the node), times prod_a (3/4 + cos(2 pi m_a / N) / 4) for TSC (1/8, 3/4, 1/8 per axis)."""
    m = np.fft.fftfreq(N) * N
    ph = [np.exp(-2j * np.pi * m * node[a] / N) for a in range(3)]
    if name == "tsc":
        ph = [p * (0.75 + 0.25 * np.cos(2 * np.pi * m / N)) for p in ph]
    return ph[0][:, None, None] * ph[1][None, :, None] * ph[2][None, None, :]


def compensated_spike_spectrum(node, N, name):
    """spike_spectrum divided by prod_a sinc(pi m_a / N)^p, p = 1, 2, 3 for NGP, CIC, TSC: the definition of the compensation.
    (It is not flat: the division undoes the continuous window, and a sampled window also holds its aliases.  A particle on a
    node with NGP or CIC is a unit spike before the compensation, not after it.)"""
    p = 1 + WINDOWS.index(name)
    s = np.sinc(np.fft.fftfreq(N)) ** p
    return spike_spectrum(node, N, name) / (s[:, None, None] * s[None, :, None] * s[None, None, :])


# ---- 4. COLA ------------------------------------------------------------------------------------------------------------------
def cola_geometries():
    """[(N, L)]: cells of 2, 1/2 and 4."""
    return [(16, 32.), (20, 10.), (32, 128.)]


def _grid(N):
    i = np.arange(N)
    return i[:, None, None], i[None, :, None], i[None, None, :]


def nyquist_wave(N, axis, A=0.25):
    """delta = A (-1)^{i_axis}: the mode m = -N/2, which the first-derivative multiplier drops: Psi1 = Psi2 = 0."""
    return A * (1. - 2. * (_grid(N)[axis] % 2)) * np.ones((N, N, N))


def two_waves(N, L, A=0.25, B=0.375, m=2):
    """(delta, psi1, psi2): delta = A (-1)^{i_x} + B cos(k y), k = 2 pi m / L.  The Nyquist wave has no first derivative and
    its own second derivative is -k_x^2 / k^2 = the wave itself, so Psi1 = (0, -B sin(k y) / k, 0), the 2LPT source is
    delta_xx delta_yy = A B (-1)^{i_x} cos(k y), a mode with k_x = pi N / L, and
    Psi2 = (0, A B k / (k_x^2 + k^2) (-1)^{i_x} sin(k y), 0)."""
    ix, iy, _ = _grid(N)
    k, kx = 2 * np.pi * m / L, np.pi * N / L
    sx = (1. - 2. * (ix % 2)) * np.ones((N, N, N))
    y = iy * (L / N)
    delta = A * sx + B * np.cos(k * y)
    psi1 = np.zeros((3, N, N, N))
    psi2 = np.zeros((3, N, N, N))
    psi1[1] = -B * np.sin(k * y) / k
    psi2[1] = A * B * k / (kx * kx + k * k) * sx * np.sin(k * y)
    return delta, psi1, psi2


def gaussian_field(N, seed=3):
    return 0.1 * np.random.RandomState(seed + N).normal(size=(N, N, N))


def init_displacements(N, L):
    """(psi1, psi2, want, special): dyadic displacements with d1 = d2 = 1, Psi1 + Psi2 = target - q.  Five particles per axis are
    sent to exactly 0 by a displacement of -q, to L, to -2.5 L, to +3.25 L and, from q = 0, by -0.0 (stays at 0) and, a sixth,
    by -2^-60 cell (rounds to L, folds to 0); ``special`` lists (particle, axis, name).  The rest move by multiples of an eighth
    of a cell within +-2 L.  want: the positions in [0, L), exact."""
    cell = L / N
    rs = np.random.RandomState(40 + N)
    e = rs.randint(-16 * N, 16 * N + 1, (3, N, N, N))
    q = np.stack(np.meshgrid(*[np.arange(N) * cell] * 3, indexing="ij"))
    target = q + e / 8. * cell
    special = []
    cases = [("to 0", 0.), ("to L", L), ("to -2.5 L", -2.5 * L), ("to +3.25 L", 3.25 * L)]
    for a in range(3):
        for j, (name, t) in enumerate(cases):
            vox = [(3 + 2 * j + a) % N, (5 + j + 2 * a) % N, (7 + 3 * j) % N]
            target[(a,) + tuple(vox)] = t
            special.append((int(np.ravel_multi_index(vox, (N, N, N))), a, name))
    psi = target - q                                                  # exact: multiples of cell / 8 below 2^12 cells
    psi2 = np.where(rs.randint(0, 2, psi.shape) == 1, cell, -cell / 4.) * np.ones_like(psi)
    psi1 = psi - psi2
    want = np.mod(target, L)                                          # dyadic: exact
    for a in range(3):
        for jn, (name, d) in enumerate((("by -0.0", -0.0), ("by -2^-60 cell", -2. ** -60 * cell))):
            vox = [4 + jn, 6 + jn, 8 + jn]
            vox[a] = 0                                                # q = 0 on this axis
            psi1[(a,) + tuple(vox)], psi2[(a,) + tuple(vox)] = d, 0.
            want[(a,) + tuple(vox)] = 0.
            special.append((int(np.ravel_multi_index(vox, (N, N, N))), a, name))
    return psi1, psi2, want.reshape(3, -1).T.copy(), special


def tiled_positions(N, L):
    """(N^3, 3): the constructed positions of paint_positions and below_zero_positions on a cubic box, repeated to one per
    Lagrangian node (the COLA stages take N^3 particles)."""
    Ls = (L, L, L)
    p = np.concatenate([paint_positions(N, Ls)[0], below_zero_positions(N, Ls)[0], dyadic_cloud(N, Ls, 200, 9)])
    return np.tile(p, (-(-N ** 3 // p.shape[0]), 1))[:N ** 3].copy()


def kick_particles(N, L):
    """(pos (N^3, 3), m, f): particles at (m + f) cells with f a multiple of 1/8, inside the box.  The first rows per axis hold a
    particle on a node, one in the last cell (nodes N - 1 and 0), one on node N - 1 and one on node 0."""
    rs = np.random.RandomState(60 + N)
    m = rs.randint(0, N, (N ** 3, 3))
    f = rs.randint(0, 8, (N ** 3, 3)) / 8.
    for a in range(3):
        m[4 * a:4 * a + 4, a] = [5, N - 1, N - 1, 0]
        f[4 * a:4 * a + 4, a] = [0., 0.625, 0., 0.]
    return (m + f) * (L / N), m, f


def linear_force(N, slope=0.5):
    """F_c = slope * (node index along axis c): (3, N, N, N)."""
    g = _grid(N)
    return np.stack([slope * g[c] * np.ones((N, N, N)) for c in range(3)])


def linear_readout(m, f, N, slope=0.5):
    """What the CIC read-out of linear_force is at (m + f) cells, by construction: the linear function itself away from the
    seam; in the last cell the interpolation between node N - 1 and node 0, (1 - f) slope (N - 1)."""
    return np.where(m + 1 < N, slope * (m + f), (1. - f) * slope * (N - 1))


def sum_bound(*terms):
    """16 * 2^-53 * (sum of the magnitudes of the terms): the bound on a floating-point sum of up to 16 products evaluated in
    another order or with other intermediate roundings (each of at most 15 additions and 16 products contributes one relative
    rounding of 2^-53 to a partial sum no larger than the sum of the magnitudes; 16 covers the eight-term CIC read-out with its
    two weight products per term as well as the three-term kick, drift and velocity expressions)."""
    return 16. * 2. ** -53 * sum(np.abs(t) for t in terms)


def storage_bound(x, dtype):
    """One unit in the last place of the stored type: 2^-23 |x| for float32 (and the smallest subnormal, below which fp32 rounds
    absolutely), 2^-52 |x| for float64.  The device and the statement each round their own fp64 value, and two values that
    differ by less than the sum bound can fall on either side of a rounding boundary: a whole ulp, not half of one."""
    eps = 2. ** -23 if np.dtype(dtype) == np.float32 else 2. ** -52
    return eps * np.abs(x) + (2. ** -149 if np.dtype(dtype) == np.float32 else 0.)
