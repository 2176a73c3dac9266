"""The constructed lines of sight of the redshift-space remap: tests/test_rsd_cases_cpu.py asserts on the CPU that each line is
what it claims to be, tests/test_rsd_constructed_gpu.py tiles cubes from them and holds every line of the device's result to
the oracle (oracle.box_oracle.redshift_space_density on these few lines).

Geometry: z = linspace(-L/2, L/2, N), dz = z[1] - z[0], a fixed H(z).  A pattern is a shift q[m] in cells of sample m,
v[m] = -Hz q[m] dz; sample m then sits at (m + q[m]) mod (N - 1) cells above z[0] (the line's length is N - 1 cells, so the last
sample is the first one's periodic image).  A single-precision plan holds v in float32: it is rounded and widened again before
the oracle, the margins below and the device see it.  One density line goes with every pattern: multiples of 1/4 below 32
(exact in float32), neighbours distinct, and d[0] + d[N-1] = 3/4, so that the fill value 3/8 is no sample's value.

Patterns (E = max(1, N // 64), the cells per lane of k_rsd_cells; the other kernels take the same lines):
  rest              q = 0: every sample an exact hit; sample N-1 wraps onto sample 0, the one tie (grid point 0 may take either)
  uniform a         q = a for a in +1/4, -1/4, +3.5, -(N/2 + 1/4): one key per cell, wraps, fill at both ends.  Samples 0 and
                    N-1 would coincide to rounding (an ill-conditioned tie), so sample N-1 is moved a further 3/8 cell (a half
                    would put it on a grid point for a = 3.5 and make grid point 1 a midpoint of two keys for a = 1/4).
                    For a = 3.5 every key sits half-way between two grid points, so every grid point is the midpoint of its
                    brackets: 'nearest' is a tie there and may take either (see lines(): alt)
  collapse c0       every sample into cell c0 at c0 + (m+1)/(N+1), c0 in 0, (E-1 or 1), N/2 - 1, N-2: linear output is the fill
                    value at every grid point, nearest output d[0] up to c0 and d[N-1] above
  two clusters      even samples into cell 3E, odd ones into cell N - 3E - 1 (60E + E-1 for N = 64E), at (m+1)/(N+1); the
                    grid points between them interpolate across 57 lanes; N/2 is the midpoint of the facing ends: a tie for
                    'nearest'
  alternate         even samples at rest, odd ones shifted by +1.5: even cells hold an exact hit and a second key, odd cells
                    are empty (but cell 1, which takes the wrapped last sample)
  permute s         samples 0 .. N-2 onto a seeded permutation of the cells 0 .. N-2 at 1/4, 1/2 or 3/4 (a cell's fraction
                    and its neighbour's never add up to 1: no grid point on a midpoint); sample N-1 into sample 0's cell at 1/8
Margins (asserted by the CPU test for every N and both precisions): (i) distinct keys >= 2^-12 cell apart and every key
>= 2^-12 cell from every grid point (but for the exact hits and the tie above); (ii) two keys that bracket a grid point
>= 1/8 cell apart; (iii) the midpoint of two keys that bracket a grid point is >= 2^-12 cell from it, but for uniform +3.5 and grid point N/2 of the clusters."""
import functools

import numpy as np

from oracle import box_oracle as bo

L = 1e3
HZ = 100.0
SIZES = (16, 24, 32, 64, 96, 128, 256, 512, 1024, 2048)
MARGIN = 2.0 ** -12
BRACKET = 0.125
FILL = 0.375
UNIFORM = ("+1/4", "-1/4", "+3.5", "-(N/2+1/4)")


def cells_per_lane(N):
    return max(1, N // 64)


def grid(N):
    return np.linspace(-0.5 * L, 0.5 * L, N)


def density(N):
    m = np.arange(N)
    d = ((97 * m) % 251 - 125) / 4.0
    d[N - 1] = 32.0
    return d


def collapse_cells(N):
    E = cells_per_lane(N)
    return (0, E - 1 if E > 1 else 1, N // 2 - 1, N - 2)


def cluster_cells(N):
    E = cells_per_lane(N)
    return 3 * E, N - 3 * E - 1


def _permute_targets(N, seed):
    rs = np.random.RandomState(1000 * seed + N)
    quarters = np.empty(N - 1, dtype=np.int64)            # the fraction of the key of every cell, in quarters
    for c in range(N - 1):
        while True:                                       # (f, 1 - f) in neighbouring cells: a grid point on their midpoint
            quarters[c] = rs.randint(1, 4)
            if c == 0 or quarters[c] + quarters[c - 1] != 4:
                break
    cell = rs.permutation(N - 1)
    t = np.empty(N)
    t[:N - 1] = cell + quarters[cell] / 4.0
    t[N - 1] = cell[0] + 0.125
    return t


def shift(N, name):
    """q[m], in cells, of the pattern `name`."""
    m = np.arange(N, dtype=np.float64)
    inside = (m + 1.0) / (N + 1.0)
    kind, _, arg = name.partition(" ")
    if kind == "rest":
        return np.zeros(N)
    if kind == "uniform":
        a = {"+1/4": 0.25, "-1/4": -0.25, "+3.5": 3.5, "-(N/2+1/4)": -(N / 2 + 0.25)}[arg]
        q = np.full(N, a)
        q[N - 1] += 0.375
        return q
    if kind == "collapse":
        return int(arg) + inside - m
    if kind == "clusters":
        lo, hi = cluster_cells(N)
        return np.where(m % 2 == 0, lo, hi) + inside - m
    if kind == "alternate":
        return np.where(m % 2 == 0, 0.0, 1.5)
    if kind == "permute":
        return _permute_targets(N, int(arg)) - m
    raise ValueError(name)


def names(N, cubic=False):
    """The patterns of a cube of N cells, an odd number of them: with four lines of sight per workgroup every wave slot of
    every workgroup then meets every pattern.  cubic: the patterns a spline can go through (distinct, well-separated keys)."""
    out = ["uniform " + a for a in UNIFORM] + ["permute 1", "permute 2"]
    if not cubic:
        out = ["rest"] + out[:4] + ["collapse %d" % c for c in collapse_cells(N)] + ["clusters", "alternate"] + out[4:]
    if len(out) % 2 == 0:
        out.append("permute 3")
    return out


def positions(N, v):
    """Where the oracle puts the samples of velocity lines v (..., N): cells above z[0], in [0, N - 1)."""
    z = grid(N)
    s = (z - v / HZ - z[0]) % (z[-1] - z[0])
    return s / (z[1] - z[0])


@functools.lru_cache(maxsize=None)
def lines(N, precision, cubic=False):
    """dict(names, d (P, N), v (P, N), want: method -> (P, N), alt_<method> (P, N)) of the cube of N cells; arrays are
    read-only.  v is what the plan holds (rounded to float32 for 'f32'), want the oracle's result on exactly these lines.
    alt: the other value a tied grid point may take -- grid point 0 of rest (two samples on it) and, for 'nearest', the grid
    points on the midpoint of their brackets (midpoint_ties) -- and want everywhere else."""
    nm = names(N, cubic)
    z = grid(N)
    v = np.stack([-HZ * shift(N, n) * (z[1] - z[0]) for n in nm])
    if precision == "f32":
        v = v.astype(np.float32).astype(np.float64)
    d = np.repeat(density(N)[None, :], len(nm), axis=0)
    geo = bo.box_geometry(L, N)
    assert np.array_equal(geo["z"], z)
    want = {}
    for method in (("cubic",) if cubic else ("linear", "nearest")):
        want[method] = bo.redshift_space_density(geo, d[None], v[None], HZ, 0., method=method)[0]
    out = dict(names=nm, d=d, v=v, want=want)
    for method, w in want.items():
        alt = w.copy()
        for r, name in enumerate(nm):
            if name == "rest":
                alt[r, 0] = d[r, 0] + d[r, N - 1] - w[r, 0]
            if method == "nearest":
                for k, (lo, hi) in midpoint_ties(N, v[r]).items():
                    assert w[r, k] in (d[r, lo], d[r, hi])
                    alt[r, k] = d[r, lo] + d[r, hi] - w[r, k]
        out["alt_" + method] = alt
    for a in [d, v] + [out[k] for k in out if k.startswith("alt_")] + list(want.values()):
        a.setflags(write=False)
    return out


def _brackets(N, v):
    """For every grid point that is no exact hit and has a key on either side: (grid points, sample below, sample above,
    position below, position above)."""
    p = positions(N, v)
    order = np.argsort(p, kind="mergesort")
    ps = p[order]
    k = np.arange(N, dtype=np.float64)
    j = np.searchsorted(ps, k)
    above, below = np.minimum(j, N - 1), np.maximum(j, 1) - 1
    ok = (j > 0) & (j < N) & (np.abs(ps[above] - k) >= 1e-9) & (np.abs(ps[below] - k) >= 1e-9)
    return np.arange(N)[ok], order[below][ok], order[above][ok], ps[below][ok], ps[above][ok]


def midpoint_ties(N, v):
    """{grid point: (sample below, sample above)} where the grid point lies within MARGIN of the midpoint of its brackets:
    'nearest' is a tie there, in the reference too."""
    k, lo, hi, plo, phi = _brackets(N, v)
    tie = np.abs(0.5 * (plo + phi) - k) < MARGIN
    return {int(a): (int(b), int(c)) for a, b, c in zip(k[tie], lo[tie], hi[tie])}


def margins(N, name, v):
    """(smallest gap between distinct keys, smallest distance of a key that is no exact hit from a grid point, smallest
    distance of two keys that bracket a grid point, smallest distance of such a pair's midpoint from the grid point, number of
    exact hits), in cells, of one velocity line."""
    p = np.sort(positions(N, v))
    near = np.abs(p - np.rint(p))
    exact = near < 1e-9                                   # rest and alternate: exact hits by construction (to rounding)
    gaps = np.diff(p)
    distinct = gaps[gaps > 1e-9] if name == "rest" else gaps
    k, _, _, plo, phi = _brackets(N, v)
    mid = np.abs(0.5 * (plo + phi) - k)
    return (distinct.min() if distinct.size else np.inf, near[~exact].min() if (~exact).any() else np.inf,
            (phi - plo).min() if k.size else np.inf, mid.min() if k.size else np.inf, int(exact.sum()))
