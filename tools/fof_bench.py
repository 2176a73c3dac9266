"""Measurement aid (GPU): friends-of-friends halo finding on COLA particles at 256^3 (and 512^3 if memory allows), b = 0.2 --
milliseconds of the stages (binning, pair search with union-find, flattening by HIP events inside fb_fof_link; sizes + host
ordering + catalogue by the host clock around synchronising calls); the part of the link time spent in the crowded cells,
timed: the second launch of the pair search, which handles every tile beyond the first of the cells that hold more than 64
particles, has its own event pair; pair tests per second of the pair search, and the share of the pair tests that falls in
the ten densest cells (their share of the link time only if every pair test cost the same; from the cell occupancy formed
on the host, up to --cell-stats-max); and scipy's periodic k-d tree + connected_components on the COLA particles at 128^3
on the host, for scale.

    python tools/fof_bench.py [--sizes 256,512] [--reps 3] [--host-size 128] [--spacing 2.0]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, halos                         # noqa: E402

HALF_SHELL = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) >= (0, 0, 0)]


def cola(N, spacing):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * N, nsamp=N, realise_now=False, precision="f32", rng="device", seed=3)
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, seed=12, return_particles=True, inplace=False)
    return box, parts


def pair_tests(pos, L, cells):
    """(pair tests of the half shell + the cell itself, their share in the ten densest home cells, largest occupancy)"""
    nc = np.array(cells)
    idx = np.minimum((pos * (nc / np.array(L))).astype(np.int64), nc - 1)
    occ = np.bincount((idx[:, 0] * nc[1] + idx[:, 1]) * nc[2] + idx[:, 2], minlength=int(np.prod(nc))).reshape(cells)
    occ = occ.astype(np.float64)
    nb = np.zeros_like(occ)
    for a, b, c in HALF_SHELL:
        nb += np.roll(occ, (-a, -b, -c), axis=(0, 1, 2))
    per = (occ * nb).reshape(-1)
    top = np.argsort(occ.reshape(-1))[-10:]
    crowded = occ.reshape(-1) > halos.FOF_TILE
    return per.sum(), per[top].sum() / per.sum(), int(occ.max()), int(crowded.sum()), per[crowded].sum() / per.sum()


def host(N, spacing):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    box, parts = cola(N, spacing)
    pos = np.asarray(parts)
    L = (box.Lx,) * 3
    ell = halos.fof_linking_length(L, N ** 3, 0.2)
    t0 = time.time()
    pr = cKDTree(pos, boxsize=L).query_pairs(ell, output_type='ndarray')
    t1 = time.time()
    n = N ** 3
    ng, _ = connected_components(coo_matrix((np.ones(len(pr), dtype=np.int8), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    t2 = time.time()
    print("host, N = %d, one core: cKDTree.query_pairs %.0f ms (%d pairs), connected_components %.0f ms (%d groups)"
          % (N, 1e3 * (t1 - t0), len(pr), 1e3 * (t2 - t1), ng))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-size", type=int, default=128)
    ap.add_argument("--spacing", type=float, default=2.0, help="mean particle spacing in Mpc")
    ap.add_argument("--cell-stats-max", type=int, default=512)
    a = ap.parse_args()
    print("friends-of-friends on COLA particles at z = 0, b = 0.2, nmin = 20, spacing %.3g Mpc; median of %d calls" % (a.spacing, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        n = N ** 3
        L = (a.spacing * N,) * 3
        ell = halos.fof_linking_length(L, n, 0.2)
        cells = halos.fof_cells(L, ell, n)
        need = halos.fof_device_bytes(n, cells, 20) + 2 * 24 * n + 20 * 4 * n       # + the particles and the COLA state
        box = CosmoBox(cosmo=default_cosmo, box_scale=a.spacing * N, nsamp=N, realise_now=False, precision="f32", rng="device", seed=3)
        if need > box.engine.free_bytes():
            print("N = %d: skipped, %.1f GiB needed" % (N, need / 2. ** 30))
            continue
        del box
        box, parts = cola(N, a.spacing)
        box.engine.release_idle_buffers()
        rows = []
        h = None
        for _ in range(a.reps + 1):
            t = {}
            h = box.find_halos(parts, timings=t)
            rows.append([t["bin_ms"], t["link_ms"], t["flatten_ms"], t["catalogue_ms"], t["link_crowded_ms"]])
        ms = np.median(np.array(rows[1:]), axis=0)
        print("N = %d: l = %.4f Mpc, cells %s, %d groups, %d of 20 or more, largest %d, %.1f %% of the particles in them"
              % (N, ell, cells, h.n_groups_all, len(h), h.count[0] if len(h) else 0, 100. * h.count.sum() / n))
        print("  bin %.3f ms, link %.3f ms, flatten %.3f ms, sizes + order + catalogue %.3f ms; work memory %.2f GiB"
              % (ms[0], ms[1], ms[2], ms[3], halos.fof_device_bytes(n, cells, 20) / 2. ** 30))
        print("  of the link: %.3f ms (%.1f %%) in the launch for the tiles beyond the first of the cells above %d particles"
              % (ms[4], 100. * ms[4] / ms[1], halos.FOF_TILE))
        if N <= a.cell_stats_max:
            tests, share, occ, ncrowd, cshare = pair_tests(np.asarray(parts), L, cells)
            print("  %.3e pair tests -> %.3e per second; the ten densest cells (largest holds %d) take %.1f %% of them, the %d"
                  " cells above %d particles %.1f %%" % (tests, tests / (ms[1] * 1e-3), occ, 100. * share, ncrowd, halos.FOF_TILE,
                                                        100. * cshare))
        del h, parts, box
    if a.host_size:
        host(a.host_size, a.spacing)


if __name__ == "__main__":
    main()
