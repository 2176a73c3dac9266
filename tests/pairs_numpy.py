"""Host reference of the pair-count definition, used only by tests.  ``counts`` is the definition:
brute force over all pairs in row blocks with exactly the arithmetic of the device -- wrapped positions and minimum-image
differences of tests/fof_numpy.py, d^2 = (dx dx + dy dy) + dz dz, bins decided on squares, no square root.  ``tree_counts``
is an independent statement for '1d' (scipy's periodic k-d tree), equal to it where no pair sits on an edge."""
import numpy as np
from scipy.spatial import cKDTree

from tests.fof_numpy import min_image, wrap


def _blocks(pos1, pos2, L, chunk):
    """Yield (row offset, dx, dy, dz) of the minimum-image differences first[rows] - second[all]."""
    L = np.asarray(L, dtype=np.float64)
    w1 = wrap(np.asarray(pos1, dtype=np.float64).reshape(-1, 3), L)
    w2 = w1 if pos2 is None else wrap(np.asarray(pos2, dtype=np.float64).reshape(-1, 3), L)
    c2 = [np.ascontiguousarray(w2[:, c]) for c in range(3)]
    for a in range(0, w1.shape[0], chunk):
        yield (a,) + tuple(min_image(w1[a:a + chunk, c][:, None] - c2[c][None, :], L[c]) for c in range(3))


def counts(pos1, pos2, L, edges, mode='1d', Nmu=10, pimax=None, chunk=256):
    """npairs, int64 of shape (nr,), (nr, Nmu) or (nr, int(pimax)).  pos2 None: auto-counts, ordered pairs i != j; else all
    n1 n2 ordered pairs.  Radial bin b iff e2[b] <= v < e2[b + 1], e2 = edges * edges, v = d^2 ('1d', '2d') or
    r_p^2 = dx dx + dy dy ('projected').  mu bin: the number of j in 1 .. Nmu - 1 with dz dz float(Nmu Nmu) >= float(j j) d^2;
    pi bin: the number of j in 1 .. npi - 1 with dz dz >= float(j j), the pair dropped if dz dz >= pimax pimax."""
    edges = np.asarray(edges, dtype=np.float64)
    e2 = edges * edges
    nr = e2.size - 1
    nsub = 1 if mode == '1d' else (int(Nmu) if mode == '2d' else int(pimax))
    out = np.zeros(nr * nsub, dtype=np.int64)
    for a, dx, dy, dz in _blocks(pos1, pos2, L, chunk):
        rp2 = dx * dx + dy * dy
        zz = dz * dz
        d2 = rp2 + zz
        v = rp2 if mode == 'projected' else d2
        ok = (v >= e2[0]) & (v < e2[nr])
        if pos2 is None:
            i = np.arange(a, a + dx.shape[0])
            ok[i - a, i] = False                                    # a particle never pairs with itself
        v, zz, d2 = v[ok], zz[ok], d2[ok]                           # the pairs inside the edges: the rest of the work is theirs
        if mode == 'projected':
            keep = ~(zz >= float(pimax) * float(pimax))
            v, zz, d2 = v[keep], zz[keep], d2[keep]
        b = np.searchsorted(e2, v, side='right') - 1                # the largest b with e2[b] <= v
        m = np.zeros(b.shape, dtype=np.int64)
        if mode == '2d':
            lhs = zz * float(nsub * nsub)
            for j in range(1, nsub):
                m += lhs >= float(j * j) * d2
        elif mode == 'projected':
            for j in range(1, nsub):
                m += zz >= float(j * j)
        out += np.bincount(b * nsub + m, minlength=nr * nsub)
    return out.reshape((nr,) if mode == '1d' else (nr, nsub))


def edge_distances(pos1, pos2, L, edges, chunk=256):
    """(the least |d - edge| over all pairs and edges -- inf if no pair comes within 1 Mpc of the last edge -- and the number of
    ordered pairs with d^2 exactly edges[b]^2 for some b); i == j is no pair in auto-counts."""
    edges = np.asarray(edges, dtype=np.float64)
    e2 = edges * edges
    near, ties = np.inf, 0
    reach2 = (edges[-1] + 1.) ** 2                                  # a pair beyond is more than 1 Mpc from every edge
    for a, dx, dy, dz in _blocks(pos1, pos2, L, chunk):
        d2 = (dx * dx + dy * dy) + dz * dz
        real = d2 <= reach2
        if pos2 is None:
            i = np.arange(a, a + dx.shape[0])
            real[i - a, i] = False
        d2 = d2[real]
        d = np.sqrt(d2)
        if d.size:
            near = min(near, np.min(np.abs(d[:, None] - edges[None, :])))
            ties += int(np.count_nonzero(d2[:, None] == e2[None, :]))
    return near, ties


def tree_counts(pos1, pos2, L, edges):
    """'1d' counts as differences of the cumulative counts d <= edge of scipy's periodic tree: bin b holds
    edges[b] < d <= edges[b + 1], which is the definition's bin wherever no pair sits on an edge (self pairs, at d = 0,
    cancel in the difference)."""
    L = np.asarray(L, dtype=np.float64)
    t1 = cKDTree(wrap(pos1, L), boxsize=L)
    t2 = t1 if pos2 is None else cKDTree(wrap(pos2, L), boxsize=L)
    cum = np.asarray(t1.count_neighbors(t2, np.asarray(edges, dtype=np.float64)), dtype=np.int64)
    return np.diff(cum)


def cells_of(pos, L, cells):
    """Occupancy of the cells of the sweep, as fof_cell numbers them."""
    L, cells = np.asarray(L, dtype=np.float64), np.asarray(cells)
    idx = np.minimum((wrap(pos, L) * (cells / L)).astype(int), cells - 1)
    return np.bincount((idx[:, 0] * cells[1] + idx[:, 1]) * cells[2] + idx[:, 2], minlength=int(np.prod(cells)))
