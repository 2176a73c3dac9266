#!/usr/bin/env python
"""Three-point correlation multipoles of the halos of a COLA run, all on the GPU: a COLA particle-mesh realisation that keeps
its particles, friends-of-friends halos (b = 0.2, 20 members or more), then the connected zeta_l(r1, r2), l <= 4, of the halos
against uniform randoms drawn on the device (N = D - R, Szapudi & Szalay; the algorithm of Slepian & Eisenstein 2015).  Printed:
the pair-count xi(r) of the same halos in the same bins, and zeta_l on the diagonal and one bin off it.
python examples/example_three_point.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo


def main(nsamp=64, spacing=4., lmax=4):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, realise_now=False, rng="device", seed=10)

    # COLA particles and their friends-of-friends halos
    _, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    fof = box.find_halos(particles, linking_length=0.2, nmin=20)

    # zeta_l(r1, r2) of the halos with 20 randoms per halo, and xi(r) from the pair counts in the same bins
    edges = np.linspace(5., 45., 5)
    tp = box.three_point(fof, edges, lmax=lmax, randoms=20, seed=1)
    xi = box.pair_counts(fof, edges=edges).xi
    print("%d particles -> %d halos and %d randoms; %d ordered pairs of the joined catalogue in range"
          % (len(particles), tp.n_data, tp.n_random, tp.npairs.sum()))
    for b, r in enumerate(tp.r):
        print("  r = %5.1f Mpc: xi = %8.4f | zeta_l(r, r), l = 0 .. %d: %s" % (r, xi[b], lmax, " ".join("%9.4f" % z for z in tp.zeta[:, b, b])))
    for b in range(len(tp.r) - 1):
        print("  r1 = %5.1f, r2 = %5.1f Mpc: zeta_l = %s" % (tp.r[b], tp.r[b + 1], " ".join("%9.4f" % z for z in tp.zeta[:, b, b + 1])))
    return fof, tp, xi


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
