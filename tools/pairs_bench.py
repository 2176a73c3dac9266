"""Measurement aid (GPU): pair counts on COLA particles at z = 0 -- the auto-counts of the particles at 128^3 and 256^3 and the
cross-counts of the friends-of-friends halos of the same run with the particles, '1d', 20 logarithmic bins from --rmin to
--rmax Mpc (default 0.5 to 20) -- milliseconds of the stages (binning; the sweep, by HIP events inside fb_pair_count; the part of
the sweep in the launch for the tiles beyond the first of the cells above 64 particles) and pair tests per second of the sweep.
A pair test is one (home particle, neighbour particle) distance: the cell itself and the 13 cells of the half shell for
auto-counts, all 27 cells for cross-counts, from the cell occupancy formed on the host -- the count tools/fof_bench.py uses
for the friends-of-friends link.  And scipy's periodic k-d tree, count_neighbors at the same edges, on the COLA particles at
--host-size^3 on the host, for scale.

    python tools/pairs_bench.py [--sizes 128,256] [--reps 3] [--host-size 64] [--spacing 2.0] [--rmin 0.5] [--rmax 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, halos                         # noqa: E402

OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


def cola(N, spacing):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * N, nsamp=N, realise_now=False, precision="f32", rng="device", seed=3)
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, seed=12, return_particles=True, inplace=False)
    return box, parts


def occupancy(pos, L, cells):
    nc = np.array(cells)
    idx = np.minimum((pos * (nc / np.array(L))).astype(np.int64), nc - 1)
    return np.bincount((idx[:, 0] * nc[1] + idx[:, 1]) * nc[2] + idx[:, 2], minlength=int(np.prod(nc))).reshape(cells).astype(np.float64)


def pair_tests(home, other, half):
    """pair tests of a sweep: every home particle against the particles of its own cell and of the neighbour cells visited
    (cells >= 3 per axis here, so the 27 offsets are distinct cells)"""
    nb = np.zeros_like(other)
    for a, b, c in OFFSETS:
        if not half or (a, b, c) >= (0, 0, 0):
            nb += np.roll(other, (-a, -b, -c), axis=(0, 1, 2))
    return float((home * nb).sum())


def timed(box, first, second, edges, reps):
    rows, p = [], None
    for _ in range(reps + 1):
        t = {}
        p = halos.pair_counts(box, first, second=second, edges=edges, timings=t)
        rows.append([t["bin_ms"], t["count_ms"], t["count_crowded_ms"]])
    return p, np.median(np.array(rows[1:]), axis=0), t["cells"]


def host(N, spacing, edges):
    from scipy.spatial import cKDTree
    box, parts = cola(N, spacing)
    pos = np.asarray(parts)
    L = (box.Lx,) * 3
    t0 = time.time()
    tree = cKDTree(pos, boxsize=L)
    cum = tree.count_neighbors(tree, edges)
    t1 = time.time()
    dev = halos.pair_counts(box, parts, edges=edges).npairs
    print("host, N = %d, one core: cKDTree(boxsize=).count_neighbors at the %d edges %.0f ms (%d pairs; the device counts %s)"
          % (N, edges.size, 1e3 * (t1 - t0), int(cum[-1] - cum[0]), "agree" if np.array_equal(np.diff(cum), dev) else "DIFFER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-size", type=int, default=64)
    ap.add_argument("--spacing", type=float, default=2.0, help="mean particle spacing in Mpc")
    ap.add_argument("--rmin", type=float, default=0.5)
    ap.add_argument("--rmax", type=float, default=20.)
    a = ap.parse_args()
    edges = np.geomspace(a.rmin, a.rmax, 21)
    print("pair counts on COLA particles at z = 0, spacing %.3g Mpc, '1d', 20 logarithmic bins from %.3g to %.3g Mpc; median of %d calls"
          % (a.spacing, a.rmin, a.rmax, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        n = N ** 3
        L = (a.spacing * N,) * 3
        box, parts = cola(N, a.spacing)
        fof = box.find_halos(parts)
        box.engine.release_idle_buffers()
        pos = np.asarray(parts)
        p, ms, cells = timed(box, parts, None, edges, a.reps)
        occ = occupancy(pos, L, cells)
        tests = pair_tests(occ, occ, min(cells) >= 3)
        print("N = %d auto: %d particles, cells %s (largest holds %d), %.4e pairs counted; work memory %.2f GiB"
              % (N, n, cells, occ.max(), p.npairs.sum(), halos.pair_device_bytes(n, 0, cells, 20) / 2. ** 30))
        print("  bin %.3f ms, sweep %.3f ms (%.3f ms of it in the launch for the tiles beyond the first); %.3e pair tests -> %.3e per second"
              % (ms[0], ms[1], ms[2], tests, tests / (ms[1] * 1e-3)))
        p, ms, cells = timed(box, fof, parts, edges, a.reps)
        tests = pair_tests(occupancy(np.asarray(fof), L, cells), occupancy(pos, L, cells), False)
        print("N = %d halos x particles: %d halos of 20 or more, cells %s, %.4e pairs counted" % (N, len(fof), cells, p.npairs.sum()))
        print("  bin %.3f ms, sweep %.3f ms (%.3f ms crowded); %.3e pair tests -> %.3e per second"
              % (ms[0], ms[1], ms[2], tests, tests / (ms[1] * 1e-3)))
        print("  xi_hm / xi_mm on the last three bins: %s" % np.array2string(p.xi[-3:] / halos.pair_counts(box, parts, edges=edges).xi[-3:],
                                                                            precision=3))
        del p, fof, parts, box
    if a.host_size:
        host(a.host_size, a.spacing, edges)


if __name__ == "__main__":
    main()
