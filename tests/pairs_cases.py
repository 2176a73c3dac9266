"""The constructed pair-count cases: tests/test_pairs_cases_cpu.py asserts on the CPU the property that keeps each one from
being vacuous, tests/test_pairs_gpu.py runs them on the device.  A case is a dict: name, first (n1, 3), second (n2, 3) or
None (auto-counts), L (3,), edges, runs -- a tuple of keyword dicts (mode, Nmu, pimax), one per call -- and random (no pair
may sit within 1e-9 of an edge, so that the tree may be compared).  Positions come from tests/fof_cases.py where the issue
names them."""
import functools

import numpy as np

from tests import fof_cases as fc
from tests import pairs_numpy as pn

ALL_MODES = (dict(mode='1d'), dict(mode='2d', Nmu=10), dict(mode='projected', pimax=3))


def _case(name, first, second, L, edges, runs, random=True):
    L = (float(L),) * 3 if np.isscalar(L) else tuple(float(a) for a in L)
    first = np.ascontiguousarray(first, dtype=np.float64)
    second = None if second is None else np.ascontiguousarray(second, dtype=np.float64)
    return dict(name=name, first=first, second=second, L=L, edges=np.asarray(edges, dtype=np.float64), runs=tuple(runs), random=random)


# ---- 1: uniform points, 4 cells on every axis: the half shell ------------------------------------------------------------
def case_uniform():
    return _case("1 uniform half shell", fc.case_a()["pos"], None, 100., np.geomspace(0.5, 20., 13),
                 (dict(mode='1d'), dict(mode='2d', Nmu=10), dict(mode='projected', pimax=20)))


# ---- 2: blobs across the seam of a cuboid box, cells of several tiles ----------------------------------------------------
def case_blobs():
    return _case("2 cuboid blobs", fc.case_b()["pos"], None, fc.B_L, [0., 0.5, 1., 2., 3., 5., 7.5, 10.],
                 (dict(mode='1d'), dict(mode='2d', Nmu=4)))


# ---- 3: two cells on an axis: the double-counting trap -------------------------------------------------------------------
def _small(L, n, seed):
    return np.random.RandomState(seed).uniform(0., 1., (n, 3)) * np.asarray(L, dtype=np.float64)


def case_cells(L, rmax, cross):
    L3 = (L,) * 3 if np.isscalar(L) else L
    second = _small(L3, 150, 32) if cross else None
    return _case("3 L=%s rmax=%g %s" % (L, rmax, "cross" if cross else "auto"), _small(L3, 200, 31), second, L3,
                 np.linspace(0., rmax, 7), ALL_MODES)


def case_cells_crowded():
    """Two cells on every axis and more than one home tile in each: the further tiles meet their own cell with fewer home
    particles than neighbours."""
    return _case("3 crowded L=8 rmax=3.9 auto", _small((8., 8., 8.), 700, 33), None, 8., np.linspace(0., 3.9, 7), ALL_MODES)


# ---- 4: exact ties on dyadic coordinates ---------------------------------------------------------------------------------
TIE_EDGES = (0., 0.75, 1.0, 1.25, 2.0)


def case_lattice(cross=False):
    """6 x 6 x 6 points on multiples of 0.25 across the seam of L = 8: every d^2 is a multiple of 1/16, exact in fp64, and the
    distances 0.75, 1.0, 1.25 (the last also as 3-4-5: 0.75 and 1.0) sit exactly on edges."""
    k = 0.25 * np.arange(6)
    g = np.stack(np.meshgrid(k, k, k, indexing='ij'), axis=-1).reshape(-1, 3)
    pos = np.mod(g + np.array([7.5, 7.25, 7.0]), 8.)
    pos = pos[np.random.RandomState(4).permutation(pos.shape[0])]
    return _case("4 lattice %s" % ("cross" if cross else "auto"), pos, pos.copy() if cross else None, 8., TIE_EDGES,
                 (dict(mode='1d'), dict(mode='2d', Nmu=5), dict(mode='projected', pimax=3)), random=False)


def case_tie_pair():
    """One pair with |dz| = 0.75 and d = 1.25: mu = 0.6 exactly, m = 3 of Nmu = 5, radial bin [1.25, 2.0); and one pair with
    |dz| = 1.0, dx = 0.75: pi bin 1, r_p = 0.75 in bin [0.75, 1.0)."""
    pos = np.array([[0., 0., 0.], [1., 0., 0.75], [4., 4., 7.5], [4.75, 4., 0.5]])
    return _case("4 tie pairs", pos, None, 8., TIE_EDGES, (dict(mode='1d'), dict(mode='2d', Nmu=5), dict(mode='projected', pimax=3)),
                 random=False)


# ---- 5: coincident points and self pairs ---------------------------------------------------------------------------------
def coincident_positions():
    p = _small((8., 8., 8.), 50, 51)
    return np.concatenate([p, p[:10], p[:1]])                     # ten points doubled, one of them tripled: 61 points


def case_coincident(e0, cross):
    pos = coincident_positions()
    return _case("5 coincident e0=%g %s" % (e0, "cross" if cross else "auto"), pos, pos.copy() if cross else None, 8.,
                 [e0, 1., 2., 3.5], (dict(mode='1d'), dict(mode='2d', Nmu=10)), random=False)


COINCIDENT_ORDERED_PAIRS = 9 * 2 + 3 * 2                          # nine doubles, one triple


# ---- 6: cross-counts of unequal catalogues -------------------------------------------------------------------------------
def case_unequal(swap=False):
    a, b = np.random.RandomState(61).uniform(0., 100., (300, 3)), fc.case_a()["pos"]
    return _case("6 unequal %s" % ("4096 x 300" if swap else "300 x 4096"), b if swap else a, a if swap else b, 100.,
                 np.geomspace(0.5, 20., 13), (dict(mode='1d'), dict(mode='2d', Nmu=10)))


# ---- 7: positions outside [0, L) -----------------------------------------------------------------------------------------
OUTSIDE_EDGES = (0., 0.15, 0.4, 1., 5., 15.)


def case_outside(wrapped):
    pos = fc.case_f_outside()["pos"]
    if wrapped:
        pos = pn.wrap(pos, np.array([32., 32., 32.]))
    return _case("7 outside %s" % ("wrapped" if wrapped else "raw"), pos, None, 32., OUTSIDE_EDGES,
                 (dict(mode='1d'), dict(mode='2d', Nmu=10), dict(mode='projected', pimax=15)), random=False)


def all_cases():
    return [case_uniform(), case_blobs(),
            case_cells(8., 3.9, False), case_cells(8., 3.9, True), case_cells(8., 2.5, False), case_cells(8., 2.5, True),
            case_cells((8., 12., 40.), 3.9, False), case_cells((8., 12., 40.), 3.9, True), case_cells_crowded(),
            case_lattice(False), case_lattice(True), case_tie_pair(),
            case_coincident(0., False), case_coincident(0., True), case_coincident(0.5, False), case_coincident(0.5, True),
            case_unequal(False), case_unequal(True), case_outside(False), case_outside(True)]


NAMES = [c["name"] for c in all_cases()]


def index_of(name):
    return NAMES.index(name)


@functools.lru_cache(maxsize=None)
def reference(index):
    """(case, tuple of the numpy counts of its runs) of all_cases()[index], computed once and shared; arrays are read-only."""
    case = all_cases()[index]
    for a in (case["first"], case["second"], case["edges"]):
        if a is not None:
            a.setflags(write=False)
    out = []
    for kw in case["runs"]:
        c = pn.counts(case["first"], case["second"], case["L"], case["edges"], **kw)
        c.setflags(write=False)
        out.append(c)
    return case, tuple(out)
