"""Host reference of the friends-of-friends definition, used only by tests.  Two independent
statements of the groups -- the definition as an O(n^2) loop over rows, and scipy's periodic k-d tree -- and the catalogue
built from the labels in plain numpy."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def wrap(x, L):
    """x - L floor(x / L), then into [0, L): a value that lands on L becomes 0."""
    x = np.asarray(x, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    w = x - L * np.floor(x / L)
    w = np.where(w < 0., w + L, w)
    return np.where(w >= L, w - L, w)


def min_image(d, L):
    h = 0.5 * L
    return np.where(d > h, d - L, np.where(d < -h, d + L, d))


def _roots(n, rows, cols):
    """Least member index of every particle's component in the graph with the given edges."""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    g = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    first = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab]


def groups_loop(pos, L, ell, chunk=256):
    """The definition: (roots, min over pairs of |d^2 / l^2 - 1|), d^2 = (dx dx + dy dy) + dz dz < l^2 on the minimum-image
    differences of the wrapped positions, strictly."""
    L = np.asarray(L, dtype=np.float64)
    w = wrap(pos, L)
    n = w.shape[0]
    cols_w = [np.ascontiguousarray(w[:, c]) for c in range(3)] if n else []
    rows, cols, tie = [], [], np.inf
    l2 = ell * ell
    for a in range(0, n, chunk):
        dx, dy, dz = [min_image(c[a:a + chunk, None] - c[None, :], La) for c, La in zip(cols_w, L)]
        d2 = (dx * dx + dy * dy) + dz * dz
        i = np.arange(a, min(a + chunk, n))
        near = np.abs(d2 / l2 - 1.)
        near[i - a, i] = np.inf                                  # i == j is no pair
        if n > 1:
            tie = min(tie, near.min())
        link = d2 < l2
        link[i - a, i] = False
        r, c = np.nonzero(link)
        rows.append(r + a)
        cols.append(c)
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    return _roots(n, rows, cols), tie


def tree_pairs(pos, L, ell):
    w = wrap(pos, L)
    if w.shape[0] < 2:
        return np.zeros((0, 2), dtype=np.int64)
    return cKDTree(w, boxsize=np.asarray(L, dtype=np.float64)).query_pairs(ell, output_type='ndarray')


def groups_tree(pos, L, ell):
    """The fast form: differs from the definition only for pairs at exactly l (the tree takes d <= l)."""
    pr = tree_pairs(pos, L, ell)
    return _roots(np.asarray(pos).shape[0], pr[:, 0], pr[:, 1])


def catalogue(pos, vel, roots, L, nmin):
    """dict(roots, count, labels, position, velocity, n_groups_all) of the groups with nmin members or more, by descending
    count, ties by ascending root; position = wrap(a + mean(min_image(w_i - a))), a the root's wrapped position."""
    L = np.asarray(L, dtype=np.float64)
    n = roots.size
    w = wrap(pos, L) if n else np.zeros((0, 3))
    uniq, cnt = np.unique(roots, return_counts=True)
    keep = cnt >= nmin
    uniq, cnt = uniq[keep], cnt[keep]
    order = np.lexsort((uniq, -cnt))
    uniq, cnt = uniq[order], cnt[order]
    rank = np.full(max(n, 1), -1, dtype=np.int32)
    rank[uniq] = np.arange(uniq.size, dtype=np.int32)
    labels = rank[roots] if n else np.zeros(0, dtype=np.int32)
    com = np.zeros((uniq.size, 3))
    vm = np.zeros((uniq.size, 3)) if vel is not None else None
    for g, r in enumerate(uniq):
        m = np.nonzero(roots == r)[0]
        a = w[r]
        com[g] = wrap(a + np.mean(min_image(w[m] - a, L), axis=0), L)
        if vel is not None:
            vm[g] = np.mean(np.asarray(vel)[m], axis=0)
    return dict(roots=uniq.astype(np.int64), count=cnt.astype(np.int64), labels=labels, position=com, velocity=vm,
                n_groups_all=int(np.unique(roots).size))
