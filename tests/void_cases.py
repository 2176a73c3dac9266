"""Constructed fields and label arrays for the void kernels (numpy only): the cases that realised Gaussian densities never
produce -- one long descent path, every voxel a minimum, plateaus, label runs that end before, on and after a wave boundary,
absent labels, a chain of N^2 regions numbered against the grain, adjacency that must not be seen.  Every value is a small
integer or a dyadic fraction, so it is the same number in fp32 and fp64.  tests/test_void_cases_cpu.py holds each builder to
tests/voids_numpy.py and asserts the property that keeps it from being vacuous; tests/test_voids_constructed_gpu.py runs them
on the device."""
import numpy as np

RUNS = (1, 3, 63, 64, 65, 257)
ORDERS = ("identity", "reversed", "zigzag", "random")


# ---- fields for the watershed ------------------------------------------------------------------------------------------------
def corridor(N):
    """(f, inside, length): one serpentine corridor, one voxel wide.  Even ix planes hold the even iy rows; consecutive rows are
    joined by one voxel at alternating z ends, consecutive planes by one voxel at the end of the last row.  f = -position along
    the corridor, so every voxel's only lower neighbour is the next one: a single descent path of ``length`` voxels.  Outside
    the corridor f = -2 length, below every voxel inside: a mask that is ignored changes every label."""
    path = []
    ys = list(range(0, N, 2))
    z = 0
    for p, ix in enumerate(range(0, N, 2)):
        rows = ys if p % 2 == 0 else ys[::-1]
        for r, iy in enumerate(rows):
            path += [(ix, iy, k) for k in (range(N) if z == 0 else range(N - 1, -1, -1))]
            z = N - 1 - z
            if r + 1 < len(rows):
                path.append((ix, (iy + rows[r + 1]) // 2, z))
        if ix + 2 < N:
            path.append((ix + 1, rows[-1], z))
    length = len(path)
    ix, iy, iz = np.array(path).T
    f = np.full((N, N, N), -2. * length)
    ins = np.zeros((N, N, N), dtype=bool)
    f[ix, iy, iz] = -np.arange(length, dtype=np.float64)
    ins[ix, iy, iz] = True
    return f, ins, length


def _parity(N):
    i = np.arange(N)
    return (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2


def checkerboard(N):
    """f = (ix + iy + iz) % 2: every even voxel is a minimum, N^3 / 2 regions (N even)."""
    return _parity(N).astype(np.float64)


def constant(N, value):
    return np.full((N, N, N), float(value))


def signed_zeros(N):
    """+0.0 on even voxels, -0.0 on odd ones: one plateau, since -0 == +0."""
    return np.where(_parity(N) == 0, 0.0, -0.0)


def ramp(N):
    """f = ix + iy + iz: one region; every interior voxel has three equal least neighbours, told apart by the index."""
    i = np.arange(N, dtype=np.float64)
    return i[:, None, None] + i[None, :, None] + i[None, None, :]


def jump_rounds(parent):
    """Rounds of pointer jumping (p <- p[p]) that move some pointer, for the flat parents of voids_numpy.descend."""
    p = parent.copy()
    ins = p >= 0
    rounds = 0
    while True:
        q = p.copy()
        q[ins] = p[p[ins]]
        if np.array_equal(q, p):
            return rounds
        p, rounds = q, rounds + 1


# ---- labels and fields for the statistics ----------------------------------------------------------------------------------
def striped_labels(N, run, nlab, zeros=False, gaps=False):
    """(labels int32, n_labels): runs of ``run`` consecutive voxels in memory order, lab.flat[i] = 1 + (i // run) % nlab.
    ``zeros``: the cycle also holds label 0, (i // run) % (nlab + 1).  ``gaps``: the nlab labels are 2, 5, 8, ... of 1..3 nlab,
    so two thirds of the labels, the first and the last among them, are absent."""
    k = np.arange(N ** 3, dtype=np.int64) // run
    if zeros:
        lab = k % (nlab + 1)
    else:
        lab = 1 + k % nlab
    n = nlab
    if gaps:
        lab = np.where(lab > 0, 3 * lab - 1, 0)
        n = 3 * nlab
    return lab.astype(np.int32).reshape(N, N, N), n


def run_end_lanes(N, run):
    """The lanes (i % 64) of the last voxel of every run of striped_labels(N, run, nlab >= 2), the box's last voxel included."""
    n = N ** 3
    ends = np.arange(run - 1, n, run)
    return set(((ends % 64).tolist())) | {(n - 1) % 64}


def dyadic_field(N, seed, lab=None, cancel=None):
    """Integers of [-2^15, 2^15] times 2^-8, both signs and zeros.  With ``lab`` and ``cancel``: the voxels of that label hold
    pairs (v, -v) (and one 0 if their number is odd), so the label's sum is exactly 0 while its weights are not."""
    rs = np.random.RandomState(seed)
    f = rs.randint(-2 ** 15, 2 ** 15 + 1, size=N ** 3).astype(np.float64) / 256.
    f[rs.choice(N ** 3, N ** 3 // 16, replace=False)] = 0.
    if cancel is not None:
        sel = np.nonzero(np.asarray(lab).reshape(-1) == cancel)[0]
        sel = sel[rs.permutation(sel.size)]
        h = sel.size // 2
        v = np.abs(f[sel[:h]]) + 1. / 256.
        f[sel[:h]], f[sel[h:2 * h]] = v, -v
        f[sel[2 * h:]] = 0.
    return f.reshape(N, N, N)


def spike_field(N, seed):
    """(f, index): integers of [-2^8, 2^8] times 2^-8 (unit scale) and one voxel, flat ``index``, of 2^40; give that voxel a label
    of its own."""
    rs = np.random.RandomState(seed)
    f = rs.randint(-2 ** 8, 2 ** 8 + 1, size=N ** 3).astype(np.float64) / 256.
    index = int(rs.randint(N ** 3 // 4, 3 * N ** 3 // 4))
    f[index] = 2.0 ** 40
    return f.reshape(N, N, N), index


def exact_sums(lab, n_labels, f):
    """sum f, sum w and sum w index per label in integer arithmetic (f a multiple of 2^-8), as fp64: what every correct
    summation of a dyadic field must give bit for bit."""
    N = lab.shape[0]
    l = lab.reshape(-1).astype(np.int64)
    v = np.rint(np.asarray(f, dtype=np.float64).reshape(-1) * 256.).astype(np.int64)
    assert np.array_equal(v / 256., np.asarray(f, dtype=np.float64).reshape(-1))
    w = np.maximum(-v, 0)
    coord = np.unravel_index(np.arange(N ** 3, dtype=np.int64), (N, N, N))

    def isum(x):
        out = np.zeros(n_labels + 1, dtype=np.int64)
        np.add.at(out, l, x)
        assert np.all(np.abs(out) < 2 ** 53)
        return out / 256.

    return dict(sum=isum(v), weight_sum=isum(w), weighted_index_sum=np.column_stack([isum(w * c) for c in coord]))


# ---- labels and fields for the merge -----------------------------------------------------------------------------------------
def chain_order(n, order, seed=7):
    """The labels 1..n along the chain: identity, reversed, zigzag (1, n, 2, n - 1, ...) or a seeded random permutation."""
    if order == "identity":
        return np.arange(1, n + 1)
    if order == "reversed":
        return np.arange(n, 0, -1)
    if order == "zigzag":
        out = np.empty(n, dtype=np.int64)
        out[0::2] = np.arange(1, (n + 1) // 2 + 1)
        out[1::2] = np.arange(n, (n + 1) // 2, -1)
        return out
    if order == "random":
        return 1 + np.random.RandomState(seed).permutation(n)
    raise ValueError(order)


def chain_labels(N, order, equal_at=None):
    """(labels int32, f, n_labels): one label per (ix, iy) column.  f is constant per column and equal to the column's position
    along a boustrophedon through the (ix, iy) plane, so consecutive columns differ by 1 and every other adjacent pair by 3 or
    more: with threshold 1.5 the whole plane is one chain of N^2 regions.  ``order`` numbers the labels along the chain
    (chain_order).  ``equal_at`` = k: positions >= k are raised by 0.5, so the interface k-1 | k differs by exactly 1.5."""
    ix, iy = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    pos = ix * N + np.where(ix % 2 == 0, iy, N - 1 - iy)
    val = pos.astype(np.float64)
    if equal_at is not None:
        val = val + 0.5 * (pos >= equal_at)
    lab = chain_order(N * N, order)[pos].astype(np.int32)
    shape = (N, N, N)
    return np.ascontiguousarray(np.broadcast_to(lab[:, :, None], shape)), np.ascontiguousarray(np.broadcast_to(val[:, :, None], shape)), N * N


def diagonal_labels(N):
    """Label 1 in one voxel, label 2 in the 20 voxels of its 3 x 3 x 3 cube that share only an edge or a corner with it."""
    lab = np.zeros((N, N, N), dtype=np.int32)
    c = N // 2
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1
        if np.count_nonzero(d) >= 2:
            lab[tuple(c + d)] = 2
    lab[c, c, c] = 1
    return lab


def face_labels(N, axis):
    """Label 1 on the face index N-1 of ``axis`` and label 2 on its face index 0, 0 between.  For axis 2 (1) the two are i and
    i + 1 (i + N) in memory wherever a row (plane) ends; for axis 0 they are neighbours only in a periodic box."""
    lab = np.zeros((N, N, N), dtype=np.int32)
    v = np.moveaxis(lab, axis, 0)
    v[N - 1] = 1
    v[0] = 2
    return lab


def sheet_labels(N):
    """Label 1 below and label 2 above a one-voxel sheet of 0 (a region outside the mask joins nothing)."""
    lab = np.zeros((N, N, N), dtype=np.int32)
    lab[:N // 2] = 1
    lab[N // 2 + 1:] = 2
    return lab


# ---- stacking ----------------------------------------------------------------------------------------------------------------
def linear_field(coef, box):
    """f = a x + b y + c z + d on the box's own coordinates."""
    a, b, c, d = coef
    return a * box.x[:, None, None] + b * box.y[None, :, None] + c * box.z[None, None, :] + d


def linear_stack(coef, centres, radii, box, grid_scale, grid_pix, swap=False):
    """(mean, count) of stacking linear_field under label 1 everywhere, from the formula alone: output [a, b, c] is the point
    c_v + R_v (grid[b], grid[a], grid[c]), valid when floor(u) lies in 0..N-2 on every axis, and a trilinear interpolant
    reproduces a linear field.  ``swap``: the mutation grid[a] <-> grid[b]."""
    N = len(box.x)
    grid = np.linspace(-grid_scale, grid_scale, grid_pix)
    ga, gb, gc = np.meshgrid(grid, grid, grid, indexing="ij")
    g = (ga, gb, gc) if swap else (gb, ga, gc)
    x0 = np.array([box.x[0], box.y[0], box.z[0]])
    dx = np.array([box.x[1], box.y[1], box.z[1]]) - x0
    tot, cnt = np.zeros(ga.shape), np.zeros(ga.shape, dtype=np.int64)
    for cen, R in zip(centres, radii):
        p = [cen[k] + R * g[k] for k in range(3)]
        ok = np.ones(ga.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            for k in range(3):
                fu = np.floor((p[k] - x0[k]) / dx[k])
                ok &= (fu >= 0) & (fu <= N - 2)
        val = coef[0] * p[0] + coef[1] * p[1] + coef[2] * p[2] + coef[3]
        tot += np.where(ok, val, 0.)
        cnt += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, tot / cnt, np.nan), cnt


def edge_u(box, axis, k):
    """(below, at): the least coordinate ``at`` on ``axis`` whose fractional index u = (c - x0) / dx, as the stacking forms it
    in fp64, is >= k, and its predecessor ``below`` (u < k).  Where k dx is hit exactly, u(at) == k."""
    x0 = (box.x, box.y, box.z)[axis][0]
    dx = (box.x, box.y, box.z)[axis][1] - x0
    c = x0 + dx * k
    for _ in range(64):
        if (c - x0) / dx < k:
            break
        c = np.nextafter(c, -np.inf)
    for _ in range(64):
        up = np.nextafter(c, np.inf)
        if (up - x0) / dx >= k:
            assert (c - x0) / dx < k and np.floor((up - x0) / dx) == k
            return c, up
        c = up
    raise AssertionError("no edge at u == %r" % k)
