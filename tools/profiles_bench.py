"""Measurement aid (GPU): halo profiles and spherical-overdensity masses on COLA particles at z = 0 and the friends-of-friends
halos found in them -- milliseconds of the binning (HIP events inside fb_profile_bin), of the profile sweep and of the
aperture sweep (host clock round the synchronising calls) and the pair tests per second of the two sweeps.  A pair test is one
(centre, particle) distance: every centre against the particles of the 27 cells round its own, from the cell occupancy formed
on the host, as tools/pairs_bench.py counts them.  The yardstick, in the same run on the same inputs: fb_pair_count
cross-counting centres x particles with the same edges in the same cells, which tests the same pairs and sums them over the
centres.  And scipy's periodic k-d tree, query_ball_point(return_length=True) at the same edges round the halos of the COLA
particles at --host-size^3, on the host, for scale.

    python tools/profiles_bench.py [--sizes 128,256] [--reps 3] [--host-size 128] [--spacing 2.0] [--rmin 0.25] [--rmax 5] [--nbins 32]"""
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


def pair_tests(home, other):
    """every home point against the points of its own cell and the 26 round it (cells >= 3 per axis here)"""
    nb = np.zeros_like(other)
    for a, b, c in OFFSETS:
        nb += np.roll(other, (-a, -b, -c), axis=(0, 1, 2))
    return float((home * nb).sum())


def host(N, spacing, edges):
    from scipy.spatial import cKDTree
    box, parts = cola(N, spacing)
    fof = box.find_halos(parts)
    pos, cen = np.asarray(parts), np.asarray(fof)
    L = (box.Lx,) * 3
    t0 = time.time()
    tree = cKDTree(pos, boxsize=L)
    cum = np.stack([tree.query_ball_point(cen, float(e), return_length=True) for e in edges], axis=1)
    t1 = time.time()
    dev = halos.halo_profiles(box, fof, parts, edges).enclosed
    print("host, N = %d, one core: cKDTree(boxsize=).query_ball_point round %d halos at the %d edges %.0f ms (the device counts %s)"
          % (N, len(fof), edges.size, 1e3 * (t1 - t0), "agree" if np.array_equal(cum, dev) else "differ in %d of %d entries"
             % (np.count_nonzero(cum != dev), dev.size)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-size", type=int, default=128)
    ap.add_argument("--spacing", type=float, default=2.0, help="mean particle spacing in Mpc")
    ap.add_argument("--rmin", type=float, default=0.25)
    ap.add_argument("--rmax", type=float, default=5.)
    ap.add_argument("--nbins", type=int, default=32)
    a = ap.parse_args()
    edges = np.geomspace(a.rmin, a.rmax, a.nbins + 1)
    print("halo profiles and SO masses on COLA particles at z = 0, spacing %.3g Mpc, %d logarithmic bins from %.3g to %.3g Mpc; "
          "median of %d calls" % (a.spacing, a.nbins, a.rmin, a.rmax, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        n = N ** 3
        L = (a.spacing * N,) * 3
        box, parts = cola(N, a.spacing)
        fof = box.find_halos(parts)
        box.engine.release_idle_buffers()
        rows, so = [], None
        for _ in range(a.reps + 1):
            t = {}
            so = halos.spherical_overdensity(box, fof, parts, edges=edges, timings=t)
            rows.append([t["bin_ms"], t["profile_ms"], t["aperture_ms"]])
        ms, cells = np.median(np.array(rows[1:]), axis=0), t["cells"]
        occ_h, occ_p = occupancy(np.asarray(fof), L, cells), occupancy(np.asarray(parts), L, cells)
        tests = pair_tests(occ_h, occ_p)
        print("N = %d: %d particles, %d halos of 20 or more, cells %s (largest holds %d), %d with an R_200; work memory %.2f GiB"
              % (N, n, len(fof), cells, occ_p.max(), np.count_nonzero(so.status == 0),
                 halos.profile_device_bytes(n, len(fof), cells, a.nbins, velocities=True) / 2. ** 30))
        print("  bin %.3f ms, profile sweep %.3f ms, aperture sweep %.3f ms; %.3e pair tests -> %.3e and %.3e per second"
              % (ms[0], ms[1], ms[2], tests, tests / (ms[1] * 1e-3), tests / (ms[2] * 1e-3)))
        rows = []
        for _ in range(a.reps + 1):
            t = {}
            p = halos.pair_counts(box, fof, second=parts, edges=edges, timings=t)
            rows.append([t["bin_ms"], t["count_ms"], t["count_crowded_ms"]])
        ms2 = np.median(np.array(rows[1:]), axis=0)
        assert t["cells"] == cells and np.array_equal(p.npairs, so.profiles.counts.sum(axis=0))
        print("  yardstick, fb_pair_count halos x particles, same edges and cells: bin %.3f ms, sweep %.3f ms (%.3f ms crowded) -> "
              "%.3e pair tests per second; profile sweep / yardstick = %.2f" % (ms2[0], ms2[1], ms2[2], tests / (ms2[1] * 1e-3), ms2[1] / ms[1]))
        del so, p, fof, parts, box
    if a.host_size:
        host(a.host_size, a.spacing, edges)


if __name__ == "__main__":
    main()
