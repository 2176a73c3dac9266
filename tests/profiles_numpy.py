"""Host reference of the halo-profile, aperture and spherical-overdensity definitions, used only by
tests.  ``profiles`` and ``apertures`` are the definitions: brute force over all (centre, particle) pairs with exactly the
arithmetic of the device -- wrapped positions and minimum-image differences of tests/fof_numpy.py, d = particle - centre,
d^2 = (dx dx + dy dy) + dz dz, every test on squares, no square root.  ``tree_profiles`` is an independent statement (scipy's
periodic k-d tree), equal to it where no particle sits on an edge.  ``so_statement`` is the spherical-overdensity finish as a
loop over centres with math.log, written apart from the product's vectorised one."""
import math

import numpy as np
from scipy.spatial import cKDTree

from tests.fof_numpy import min_image, wrap


def _blocks(centres, pos, L, chunk=256):
    """Yield (row offset, dx, dy, dz), each (rows, n): the minimum-image differences particle - centre."""
    L = np.asarray(L, dtype=np.float64)
    wc = wrap(np.asarray(centres, dtype=np.float64).reshape(-1, 3), L)
    wp = wrap(np.asarray(pos, dtype=np.float64).reshape(-1, 3), L)
    cols = [np.ascontiguousarray(wp[:, c]) for c in range(3)]
    for a in range(0, wc.shape[0], chunk):
        yield (a,) + tuple(min_image(cols[c][None, :] - wc[a:a + chunk, c][:, None], L[c]) for c in range(3))


def profiles(centres, pos, L, edges):
    """(inner (nh,), counts (nh, nr)), int64: inner = #{d^2 < e0^2}, counts[b] = #{e_b^2 <= d^2 < e_{b+1}^2}."""
    edges = np.asarray(edges, dtype=np.float64)
    e2 = edges * edges
    nh, nr = np.asarray(centres).reshape(-1, 3).shape[0], e2.size - 1
    inner, counts = np.zeros(nh, dtype=np.int64), np.zeros((nh, nr), dtype=np.int64)
    for a, dx, dy, dz in _blocks(centres, pos, L):
        d2 = (dx * dx + dy * dy) + dz * dz
        col = np.searchsorted(e2, d2, side='right')               # 0: below e0; b + 1: bin b; nr + 1: at or beyond the last edge
        for i in range(d2.shape[0]):
            row = np.bincount(col[i], minlength=nr + 2)
            inner[a + i], counts[a + i] = row[0], row[1:nr + 1]
    return inner, counts


def tree_profiles(centres, pos, L, edges):
    """The (nh, nr + 1) cumulative counts #{d <= e_j} of scipy's periodic tree: N(< e_j) of the definition wherever no
    particle sits on an edge."""
    L = np.asarray(L, dtype=np.float64)
    tree = cKDTree(wrap(pos, L), boxsize=L)
    wc = wrap(np.asarray(centres, dtype=np.float64).reshape(-1, 3), L)
    return np.stack([np.asarray(tree.query_ball_point(wc, float(e), return_length=True), dtype=np.int64) for e in edges], axis=1)


def fx_bits(bound):
    """Fractional bits of a two-word fixed-point sum whose magnitude stays below ``bound``: 93 - e, bound < 2^e (frexp)."""
    return 93 - (math.frexp(bound)[1] if bound > 0. else 0)


def apertures(centres, pos, L, r2, vel=None):
    """dict(count, com, vmean, svv, sigma_v): per centre the particles with d^2 < r2 strictly; com = wrap(c + fsum(d) / m),
    vmean = fsum(v) / m, svv = fsum((vx vx + vy vy) + vz vz) / m, sigma_v = sqrt(max(0, (svv - vmean.vmean) / 3)); NaN
    where m = 0.  The sums are correctly rounded (math.fsum)."""
    L = np.asarray(L, dtype=np.float64)
    wc = wrap(np.asarray(centres, dtype=np.float64).reshape(-1, 3), L)
    nh = wc.shape[0]
    out = dict(count=np.zeros(nh, dtype=np.int64), com=np.full((nh, 3), np.nan), vmean=np.full((nh, 3), np.nan),
               svv=np.full(nh, np.nan), sigma_v=np.full(nh, np.nan))
    v = None if vel is None else np.asarray(vel, dtype=np.float64)
    for a, dx, dy, dz in _blocks(centres, pos, L):
        d2 = (dx * dx + dy * dy) + dz * dz
        for i in range(d2.shape[0]):
            h = a + i
            m = np.nonzero(d2[i] < r2[h])[0]
            out["count"][h] = m.size
            if not m.size:
                continue
            mean = np.array([math.fsum(d[i][m]) / m.size for d in (dx, dy, dz)])
            out["com"][h] = wrap(wc[h] + mean, L)
            if v is not None:
                vm = np.array([math.fsum(v[m, c]) / m.size for c in range(3)])
                q = (v[m, 0] * v[m, 0] + v[m, 1] * v[m, 1]) + v[m, 2] * v[m, 2]
                out["vmean"][h], out["svv"][h] = vm, math.fsum(q) / m.size
                out["sigma_v"][h] = math.sqrt(max(0., (out["svv"][h] - ((vm[0] * vm[0] + vm[1] * vm[1]) + vm[2] * vm[2])) / 3.))
    return out


def so_statement(edges, inner, counts, particle_mass, rho_ref, delta):
    """(radius, mass, status) of every centre, as the issue states it: N(< e_j) = inner + sum_{b < j} counts; rho_j =
    particle_mass N / (4 pi / 3 e_j^3) at e_j > 0; j* the largest j with rho_j >= delta rho_ref; none: status 1; the last
    edge: status 2; else log-log interpolation between j* and j* + 1."""
    nh, nr = counts.shape
    radius, mass, status = np.full(nh, np.nan), np.full(nh, np.nan), np.zeros(nh, dtype=np.int64)
    thr = delta * rho_ref
    for h in range(nh):
        N = [int(inner[h])]
        for b in range(nr):
            N.append(N[-1] + int(counts[h, b]))
        rho = [particle_mass * N[j] / (4. * math.pi / 3. * edges[j] ** 3) if edges[j] > 0. else None for j in range(nr + 1)]
        js = [j for j in range(nr + 1) if rho[j] is not None and rho[j] >= thr]
        if not js:
            status[h] = 1
        elif js[-1] == nr:
            status[h] = 2
        else:
            j = js[-1]
            t = (math.log(thr) - math.log(rho[j])) / (math.log(rho[j + 1]) - math.log(rho[j]))
            radius[h] = math.exp(math.log(edges[j]) + t * (math.log(edges[j + 1]) - math.log(edges[j])))
            mass[h] = 4. * math.pi / 3. * thr * radius[h] ** 3
    return radius, mass, status
