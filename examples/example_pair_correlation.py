#!/usr/bin/env python
"""Small-scale clustering of the halos of a COLA run by pair counts, all on the GPU: a COLA particle-mesh realisation that
keeps its particles, friends-of-friends halos of the particles, then the halo auto-correlation, the halo-matter
cross-correlation and the matter auto-correlation xi(r) from pair counts in logarithmic bins (what nbodykit's
SimulationBox2PCF gives), down to separations far below a mesh cell.  Beside them, on the bins wider than two mesh cells, the
FFT estimate ``correlation_function`` of the painted halo catalogue, which carries the assignment window and the shot noise
that the pair counts do not.  python examples/example_pair_correlation.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo


def main(nsamp=128, spacing=4., nbins=8):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, realise_now=False, rng="device", seed=10)

    # COLA particles and their friends-of-friends halos
    matter, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    halos = box.find_halos(particles, linking_length=0.2, nmin=20)
    print("%d particles, %d halos of 20 or more" % (len(particles), len(halos)))

    # Pair counts: from a quarter of the mean particle spacing to ten spacings
    edges = np.geomspace(0.25 * spacing, 10. * spacing, nbins + 1)
    hh = box.pair_counts(halos, edges=edges)
    hm = box.pair_counts(halos, second=particles, edges=edges)
    mm = box.pair_counts(particles, edges=edges)

    # The FFT estimate from the painted catalogue, on the bins it resolves
    mesh = box.paint_catalogue(halos, window='tsc', compensated=True)
    delta_h = mesh * (float(box.N) ** 3 / len(halos)) - 1.
    wide = edges >= 2. * spacing
    r_fft, xi_fft, _ = box.correlation_function(delta_h, rbins=edges[wide])
    fft = dict(zip(np.nonzero(wide)[0][:-1], xi_fft))

    print("   r [Mpc]      pairs hh   xi_hh      pairs hm   xi_hm      pairs mm   xi_mm     xi_hh (FFT of the painted halos)")
    for b in range(nbins):
        print("  %6.2f-%6.2f %9d %8.3f %13d %8.3f %13d %8.3f   %s"
              % (edges[b], edges[b + 1], hh.npairs[b], hh.xi[b], hm.npairs[b], hm.xi[b], mm.npairs[b], mm.xi[b],
                 "%8.3f" % fft[b] if b in fft else "   -"))
    return halos, hh, hm, mm


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
