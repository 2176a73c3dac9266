"""Measurement aid (GPU): three-point multipole moments (fb_triplet_multipoles) on COLA particles at z = 0 -- milliseconds of the
binning, the sweep and the finish (HIP events inside the call; median, minimum and maximum of the calls after a warm-up), the
in-range pairs per second (the pairs are the call's own ``npairs``) and the Y_lm accumulations per second (pairs x (lmax + 1)^2),
for lmax = 10 and lmax = 4.  The yardstick, in the same run on the same particles and edges: fb_pair_count ('1d'), which tests
the same candidate pairs and only counts them.  And the numpy statement's harmonics and sums (tests/threepoint_numpy.py) round
the first --host-primaries particles on one host core, for scale.

    python tools/threepoint_bench.py [--size 128] [--reps 3] [--spacing 2.0] [--rmin 2] [--rmax 20] [--nbins 10] [--host-primaries 32]"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, halos                         # noqa: E402


def spread(v):
    return "%.2f (%.2f .. %.2f)" % (np.median(v), np.min(v), np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spacing", type=float, default=2.0, help="mean particle spacing in Mpc")
    ap.add_argument("--rmin", type=float, default=2.)
    ap.add_argument("--rmax", type=float, default=20.)
    ap.add_argument("--nbins", type=int, default=10)
    ap.add_argument("--lmax", default="10,4")
    ap.add_argument("--host-primaries", type=int, default=32)
    a = ap.parse_args()
    N, edges = a.size, np.linspace(a.rmin, a.rmax, a.nbins + 1)
    box = CosmoBox(cosmo=default_cosmo, box_scale=a.spacing * N, nsamp=N, realise_now=False, precision="f32", rng="device", seed=3)
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, seed=12, return_particles=True, inplace=False)
    box.engine.release_idle_buffers()
    n = len(parts)
    print("three-point multipoles of %d^3 COLA particles at z = 0, spacing %.3g Mpc, %d linear bins from %.3g to %.3g Mpc; "
          "median (min .. max) of %d calls after a warm-up" % (N, a.spacing, a.nbins, a.rmin, a.rmax, a.reps))
    rows = []
    for _ in range(a.reps + 1):
        t = {}
        pc = halos.pair_counts(box, parts, edges=edges, timings=t)
        rows.append([t["bin_ms"], t["count_ms"]])
    pr = np.array(rows[1:])
    pairs = float(pc.npairs.sum())
    print("yardstick fb_pair_count '1d': bin %s ms, sweep %s ms; %.4e ordered pairs in range -> %.3e pairs/s"
          % (spread(pr[:, 0]), spread(pr[:, 1]), pairs, pairs / (np.median(pr[:, 1]) * 1e-3)))
    for lmax in [int(x) for x in a.lmax.split(",")]:
        rows = []
        for _ in range(a.reps + 1):
            t = {}
            M, npairs, _ = halos.triplet_multipoles(box, parts, edges, lmax=lmax, timings=t)
            rows.append([t["bin_ms"], t["sweep_ms"], t["finish_ms"]])
        r = np.array(rows[1:])
        assert np.array_equal(npairs, pc.npairs) and t["cells"] == pc_cells(box, edges, n)
        sweep = np.median(r[:, 1]) * 1e-3
        print("lmax = %2d: bin %s ms, sweep %s ms, finish %s ms; cells %s, work memory %.2f GiB" % (
            lmax, spread(r[:, 0]), spread(r[:, 1]), spread(r[:, 2]), t["cells"],
            halos.triplet_device_bytes(n, t["cells"], a.nbins, lmax) / 2. ** 30))
        print("           %.3e pairs/s, %.3e Y_lm accumulations/s; sweep / pair-count sweep = %.1f"
              % (pairs / sweep, pairs * (lmax + 1) ** 2 / sweep, np.median(r[:, 1]) / np.median(pr[:, 1])))
    if a.host_primaries:
        from tests import threepoint_numpy as tn
        pos, L, lmax = np.asarray(parts), np.array([box.Lx, box.Ly, box.Lz]), 10
        e2 = edges * edges
        t0 = time.time()
        done = 0
        for i in range(a.host_primaries):
            j, b, dx, dy, dz, d2 = tn.neighbours(pos, i, L, e2)
            rr = np.sqrt(d2)
            Y = tn.harmonics(dx / rr, dy / rr, dz / rr, lmax)
            for q in range(a.nbins):
                [math.fsum(row) for row in Y[:, b == q].tolist()]
            done += j.size
        dt = time.time() - t0
        print("host, one core, the numpy statement's neighbours, harmonics (lmax = 10) and sums round %d primaries: %.2f s, "
              "%.3e pairs/s" % (a.host_primaries, dt, done / dt))


def pc_cells(box, edges, n):
    return halos.pair_cells((float(box.Lx), float(box.Ly), float(box.Lz)), (edges[-1],) * 3, n)


if __name__ == "__main__":
    main()
