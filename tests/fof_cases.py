"""The constructed friends-of-friends cases: tests/test_fof_cases_cpu.py asserts on the CPU the property that keeps each one
from being vacuous, tests/test_fof_gpu.py runs them on the device.  A case is a dict: name, pos (n, 3), vel (n, 3) or None,
L (3,), ell (the linking length passed), absolute, nmin, random (its pairs must stay clear of the linking length)."""
import functools

import numpy as np

from tests import fof_numpy as fn


def _case(name, pos, L, ell, nmin, absolute=True, vel="draw", random=True, seed=0):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    if isinstance(vel, str):
        vel = 300. * np.random.RandomState(1000 + seed).normal(size=pos.shape)
    L = (float(L),) * 3 if np.isscalar(L) else tuple(float(a) for a in L)
    return dict(name=name, pos=pos, vel=vel, L=L, ell=ell, absolute=absolute, nmin=nmin, random=random)


def length(case):
    """The linking length in Mpc."""
    if case["absolute"]:
        return float(case["ell"])
    L = case["L"]
    return float(case["ell"]) * (L[0] * L[1] * L[2] / case["pos"].shape[0]) ** (1. / 3.)


# ---- A: uniform random, relative linking length, many small groups with ties in count -----------------------------------------
def case_a():
    rs = np.random.RandomState(11)
    return _case("A uniform", rs.uniform(0., 100., (4096, 3)), 100., 0.6, 5, absolute=False, seed=1)


# ---- B: cuboid box, blobs on the seam, one crowded cell, shuffled --------------------------------------------------------------
B_L = (64., 96., 128.)
SEAM = [(0., 48., 64.), (32., 0., 64.), (32., 48., 0.), (0., 0., 64.), (0., 48., 0.), (32., 0., 0.), (0., 0., 0.),
        (63.95, 95.95, 30.)]


def case_b(shuffle_seed=5):
    rs = np.random.RandomState(23)
    L = np.array(B_L)
    centres = np.array(SEAM + [tuple(rs.uniform(4., 60., 3) * L / 64.) for _ in range(16)])
    sizes = np.concatenate([[400, 250, 160, 120, 90, 70, 60, 300], rs.randint(5, 401, 16)])
    parts = [c + 0.8 * rs.normal(size=(m, 3)) for c, m in zip(centres, sizes)]
    parts.append(rs.uniform(0., 1., (3000, 3)) * L)
    pos = np.concatenate(parts)
    pos = pos[np.random.RandomState(shuffle_seed).permutation(pos.shape[0])]
    return _case("B cuboid blobs", pos, B_L, 0.7, 20, seed=2)        # positions are NOT wrapped: blobs spill over the seam


# ---- C: large linking length: three and two cells per side ------------------------------------------------------------------
def case_c(ell):
    rs = np.random.RandomState(3)
    return _case("C ell=%g" % ell, rs.uniform(0., 8., (12, 3)), 8., ell, 1, seed=3)


# ---- D: exact ties on dyadic coordinates ------------------------------------------------------------------------------------
def case_d(ell=1.0):
    k = np.arange(40)
    x = np.mod(60. + 0.75 * k + np.where(k >= 20, 0.25, 0.), 64.)
    pos = np.stack([x, np.zeros(40), np.full(40, 63.5)], axis=1)
    return _case("D ties ell=%r" % ell, pos, 64., ell, 1, random=False, seed=4)


# ---- E: one long chain, wrapping the box 16 times -------------------------------------------------------------------------
def case_e(order="index"):
    k = np.arange(8192)
    pos = np.stack([np.mod(0.125 * k, 64.), 32. + 20. * np.cos(0.004 * k), 32. + 20. * np.sin(0.004 * k)], axis=1)
    if order == "reversed":
        pos = pos[::-1]
    elif order == "shuffled":
        pos = pos[np.random.RandomState(8).permutation(8192)]
    return _case("E chain %s" % order, pos, 64., 0.25, 20, random=False, seed=5)


# ---- F: degenerate inputs ---------------------------------------------------------------------------------------------------
def case_f_coincident():
    pos = np.array([[1., 2., 3.], [10., 10., 10.], [1., 2., 3.], [20., 5., 5.]])
    return _case("F coincident", pos, 32., 0.5, 2, random=False, seed=6)


def case_f_outside():
    """Positions outside [0, L): negative, equal to L, several boxes away; two tight clumps across the seam."""
    L = 32.
    pos = np.array([[-0.1, 5., 5.], [0.1, 5., 5.], [L, 5.2, 5.], [L + 0.2, 5., -3. * L + 5.1],       # one clump at x ~ 0
                    [16., L, 0.], [16.2, 0., L], [16.1, -1e-20, 0.1], [16., 2. * L, 64.2],           # one at y, z ~ 0
                    [8., 8., 8.]])
    return _case("F outside", pos, L, 0.5, 2, random=False, seed=7)


def case_f_tiny(n):
    return _case("F n=%d" % n, np.full((n, 3), 3.), 32., 0.5, 2, vel=None, random=False)


# ---- G: a cell grid whose scan carries a running sum across rounds ----------------------------------------------------------
G_CELLS = (128, 128, 64)                   # 2^20 cells: the scan's 2^20 + 1 outputs are 257 chunks of 4096, one more than a round


@functools.lru_cache(maxsize=None)
def case_g_many_cells():
    """(pos, L, ell, roots) for the raw link call on G_CELLS cells of the unit box (find_halos never picks so fine a grid for
    so few particles): a linked pair in cell 0, one in the last cell, one across the periodic corner between those two cells,
    294 scattered singles.  roots: the definition's."""
    ell = (1. - 2. ** -20) / 128.
    pairs = np.array([[0.004, 0.004, 0.012], [0.005, 0.004, 0.013],            # cell (0, 0, 0)
                      [0.995, 0.995, 0.988], [0.996, 0.995, 0.987],            # cell (127, 127, 63)
                      [0.001, 0.001, 0.001], [0.999, 0.999, 0.999]])           # cell 0 and the last cell, through the corner
    pos = np.concatenate([pairs, np.random.RandomState(21).uniform(0.02, 0.98, (294, 3))])
    roots = fn.groups_loop(pos, (1., 1., 1.), ell)[0]
    for v in (pos, roots):
        v.setflags(write=False)
    return pos, (1., 1., 1.), ell, roots


def all_cases():
    return [case_a(), case_b(), case_c(2.5), case_c(3.9), case_d(1.0), case_d(1.0 + 2. ** -40), case_e("index"),
            case_e("reversed"), case_e("shuffled"), case_f_coincident(), case_f_outside()]


@functools.lru_cache(maxsize=None)
def reference(index):
    """(case, catalogue of the tree form) of all_cases()[index], computed once and shared; arrays are read-only."""
    case = all_cases()[index]
    roots = exact_roots(case)
    cat = fn.catalogue(case["pos"], case["vel"], roots, case["L"], case["nmin"])
    for v in list(cat.values()) + [case["pos"], case["vel"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    cat["all_roots"] = roots
    return case, cat


def exact_roots(case):
    """Roots by the definition: the tree form where no pair sits at the linking length, else the loop."""
    if case["random"] or case["name"].startswith("E"):
        return fn.groups_tree(case["pos"], case["L"], length(case))
    return fn.groups_loop(case["pos"], case["L"], length(case))[0]


def seam_groups(case, cat):
    """Kept groups with members on both sides of a seam: wrapped coordinates both below and above half the box on an axis
    along which the group's minimum-image extent is small."""
    L = np.array(case["L"])
    w = fn.wrap(case["pos"], L)
    n = 0
    for g in range(cat["count"].size):
        m = w[cat["labels"] == g]
        across = [(m[:, a].max() - m[:, a].min() > 0.5 * L[a]) for a in range(3)]
        n += bool(any(across))
    return n
