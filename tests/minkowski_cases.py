"""Constructed bodies with known cell-complex counts for the Minkowski functionals, a brute-force cell
complex to check the numpy statement against, and the Gaussian fields of the theory check.  Validated without a GPU by
tests/test_minkowski_cases_cpu.py; the GPU tests run the kernel on the same cases.

A case is (name, field, expected): the field is 1 on the body and 0 elsewhere, the threshold is 0.5, and expected is the dict
n3, n2 (x, y, z: faces by normal), n1 (x, y, z: edges by direction), n0, chi.  Every body is also given with its axes permuted,
so that an orientation mix-up shows."""
import itertools

import numpy as np

THRESHOLD = 0.5
PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))        # the field's axis i is the body's axis perm[i]


def _body(N, voxels):
    f = np.zeros((N, N, N))
    for v in voxels:
        f[tuple(int(c) % N for c in v)] = 1.
    return f


def _box_voxels(lo, hi):
    return list(itertools.product(*[range(a, b) for a, b in zip(lo, hi)]))


def _expect(n3, n2, n1, n0, chi):
    return dict(n3=int(n3), n2=tuple(int(v) for v in n2), n1=tuple(int(v) for v in n1), n0=int(n0), chi=int(chi))


def bodies(N):
    """[(name, voxels or None for the full box, expected)] on the canonical axes.  The literal counts hold for every N >= 8; the
    plane, the rod and the full box scale with N."""
    M = N - 1
    shell = [v for v in _box_voxels((5, 5, 5), (8, 8, 8)) if v != (6, 6, 6)]
    ring = [v for v in _box_voxels((2, 3, 4), (5, 6, 5)) if v != (3, 4, 4)]
    full = _box_voxels((0, 0, 0), (N, N, N))
    return [
        ("one voxel", [(3, 4, 5)], _expect(1, (2, 2, 2), (4, 4, 4), 8, 1)),
        ("pair along x", [(3, 4, 5), (4, 4, 5)], _expect(2, (3, 4, 4), (8, 6, 6), 12, 1)),
        ("pair along x across the seam", [(M, 4, 5), (0, 4, 5)], _expect(2, (3, 4, 4), (8, 6, 6), 12, 1)),
        ("pair sharing an edge", [(3, 4, 5), (4, 5, 5)], _expect(2, (4, 4, 4), (8, 8, 7), 14, 1)),
        ("pair sharing a vertex", [(3, 4, 5), (4, 5, 6)], _expect(2, (4, 4, 4), (8, 8, 8), 15, 1)),
        ("pair sharing a vertex across the seam", [(M, M, M), (0, 0, 0)], _expect(2, (4, 4, 4), (8, 8, 8), 15, 1)),
        ("3^3 shell, centre out", shell, _expect(26, (36, 36, 36), (48, 48, 48), 64, 2)),
        ("3 x 3 ring in a z-plane", ring, _expect(8, (12, 12, 16), (24, 24, 16), 32, 0)),
        ("full z-plane", _box_voxels((0, 0, 5), (N, N, 6)),
         _expect(N * N, (N * N, N * N, 2 * N * N), (2 * N * N, 2 * N * N, N * N), 2 * N * N, 0)),
        ("rod along x", _box_voxels((0, 4, 5), (N, 5, 6)), _expect(N, (N, 2 * N, 2 * N), (4 * N, 2 * N, 2 * N), 4 * N, 0)),
        ("full box", full, _expect(N ** 3, (N ** 3,) * 3, (N ** 3,) * 3, N ** 3, 0)),
        ("full box minus one voxel", [v for v in full if v != (3, 4, 5)],
         _expect(N ** 3 - 1, (N ** 3,) * 3, (N ** 3,) * 3, N ** 3, 1)),
    ]


def cases_3d(N):
    """[(name, field, expected)]: every body on each of the three cyclic axis orders"""
    out = []
    for name, voxels, exp in bodies(N):
        base = _body(N, voxels)
        for perm in PERMS:
            # the field's axis i is the body's axis perm[i]
            e = dict(exp, n2=tuple(exp["n2"][perm[i]] for i in range(3)), n1=tuple(exp["n1"][perm[i]] for i in range(3)))
            out.append(("%s, axes %s" % (name, "".join("xyz"[p] for p in perm)), np.ascontiguousarray(base.transpose(perm)), e))
    return out


def _map(N, pixels):
    m = np.zeros((N, N))
    for p in pixels:
        m[tuple(int(c) % N for c in p)] = 1.
    return m


def shapes_2d(N):
    """[(name, map, expected)]: expected is the dict n2, n1 (x, y: edges by direction), n0, chi"""
    def exp(n2, n1, n0, chi):
        return dict(n2=int(n2), n1=tuple(int(v) for v in n1), n0=int(n0), chi=int(chi))
    ring = [p for p in itertools.product(range(2, 5), range(3, 6)) if p != (3, 4)]
    return [
        ("empty", _map(N, []), exp(0, (0, 0), 0, 0)),
        ("one pixel", _map(N, [(3, 4)]), exp(1, (2, 2), 4, 1)),
        ("one pixel on the corner", _map(N, [(N - 1, N - 1)]), exp(1, (2, 2), 4, 1)),
        ("pair along x across the seam", _map(N, [(N - 1, 4), (0, 4)]), exp(2, (4, 3), 6, 1)),
        ("pair along y", _map(N, [(3, 4), (3, 5)]), exp(2, (3, 4), 6, 1)),
        ("ring", _map(N, ring), exp(8, (12, 12), 16, 0)),
        ("full row along x", _map(N, [(i, 4) for i in range(N)]), exp(N, (2 * N, N), 2 * N, 0)),
        ("full row along y", _map(N, [(4, j) for j in range(N)]), exp(N, (N, 2 * N), 2 * N, 0)),
        ("full map", np.ones((N, N)), exp(N * N, (N * N, N * N), N * N, 0)),
    ]


def channel_cube(N):
    """(cube, expected): channel c of the cube holds shape c mod len(shapes_2d) -- different shapes in adjacent channels, so that
    a transposition of the channel axis with a pixel axis shows.  expected: dict n2 (N,), n1 (2, N), n0 (N,), chi (N,)."""
    shapes = shapes_2d(N)
    cube = np.zeros((N, N, N))
    pick = [shapes[c % len(shapes)] for c in range(N)]
    for c, (_, m, _) in enumerate(pick):
        cube[:, :, c] = m
    e = [p[2] for p in pick]
    return cube, dict(n2=np.array([x["n2"] for x in e]), n1=np.array([x["n1"] for x in e]).T, n0=np.array([x["n0"] for x in e]),
                      chi=np.array([x["chi"] for x in e]))


# ---- the cell complex by brute force ----------------------------------------------------------------------------------------
def brute_force_3d(mask):
    """The counts of the cell complex of the union of the closed voxels of a boolean (N, N, N) mask, periodic, from Python sets:
    in doubled coordinates modulo 2 N voxel (i, j, k) has its centre at (2i + 1, 2j + 1, 2k + 1) and owns the 27 points at
    offsets -1, 0, +1 (half a voxel) from it.  A point with 3 odd coordinates is a cell, with 2 a face whose normal is the even
    axis, with 1 an edge that runs along the odd axis, with none a vertex."""
    N = mask.shape[0]
    pts = set()
    for v in np.argwhere(mask):
        for d in itertools.product((-1, 0, 1), repeat=3):
            pts.add(tuple((2 * int(v[a]) + 1 + d[a]) % (2 * N) for a in range(3)))
    n3, n0, n2, n1 = 0, 0, [0, 0, 0], [0, 0, 0]
    for p in pts:
        odd = [c & 1 for c in p]
        k = sum(odd)
        if k == 3:
            n3 += 1
        elif k == 2:
            n2[odd.index(0)] += 1
        elif k == 1:
            n1[odd.index(1)] += 1
        else:
            n0 += 1
    return dict(n3=n3, n2=tuple(n2), n1=tuple(n1), n0=n0)


def brute_force_2d(mask):
    """The same for a periodic 2-D map: n2 pixels, n1 edges by the axis they run along, n0 vertices"""
    N = mask.shape[0]
    pts = set()
    for v in np.argwhere(mask):
        for d in itertools.product((-1, 0, 1), repeat=2):
            pts.add(tuple((2 * int(v[a]) + 1 + d[a]) % (2 * N) for a in range(2)))
    n2, n0, n1 = 0, 0, [0, 0]
    for p in pts:
        odd = [c & 1 for c in p]
        k = sum(odd)
        if k == 2:
            n2 += 1
        elif k == 1:
            n1[odd.index(1)] += 1
        else:
            n0 += 1
    return dict(n2=n2, n1=tuple(n1), n0=n0)


# ---- Gaussian fields of the theory check ------------------------------------------------------------------------------------
def gaussian_field(N, R, seed, dim=3):
    """(field, sigma1 / sigma0): white noise RandomState(seed).normal(size=(N,) * dim) multiplied in k-space by exp(-k^2 R^2 / 2),
    k = 2 pi fftfreq(N) per voxel, divided by its standard deviation; sigma1^2 / sigma0^2 = sum k^2 |f_k|^2 / sum |f_k|^2."""
    w = np.random.RandomState(seed).normal(size=(N,) * dim)
    k1 = 2. * np.pi * np.fft.fftfreq(N)
    k2 = sum(np.meshgrid(*([k1 ** 2] * dim), indexing="ij"))
    fk = np.fft.fftn(w) * np.exp(-0.5 * k2 * R * R)
    f = np.fft.ifftn(fk).real
    p = np.abs(fk) ** 2
    return f / np.std(f), float(np.sqrt(np.sum(k2 * p) / np.sum(p)))
