#!/usr/bin/env python
"""Halos of a COLA run and their large-scale bias, all on the GPU: a COLA particle-mesh realisation that keeps its particles,
friends-of-friends halos of the particles (b = 0.2, 20 members or more), the halo catalogue painted onto the mesh
(nbodykit's to_mesh(window='tsc', compensated=True)), the halo-matter cross spectrum against the matter spectrum, and the
bias b = P_hm / P_mm on the largest scales.  python examples/example_fof_halos.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo


def main(nsamp=128, spacing=4.):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, realise_now=False, rng="device", seed=10)

    # COLA: the matter density on the mesh and the particles behind it
    matter, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)

    # Friends-of-friends halos of the particles
    halos = box.find_halos(particles, linking_length=0.2, nmin=20)
    print("%d particles -> %d groups, %d halos of 20 or more; linking length %.3f Mpc; particle mass %.3e Msun"
          % (len(particles), halos.n_groups_all, len(halos), halos.linking_length, halos.particle_mass))
    for m, c, x, v in list(zip(halos.mass, halos.count, np.asarray(halos), np.asarray(halos.velocities)))[:5]:
        print("  M = %.3e Msun (%5d members) at (%7.2f, %7.2f, %7.2f) Mpc, v = (%6.0f, %6.0f, %6.0f) km/s" % ((m, c) + tuple(x) + tuple(v)))

    # Halo overdensity on the mesh, halo-matter and matter-matter spectra
    mesh = box.paint_catalogue(halos, window='tsc', compensated=True)
    delta_h = mesh * (float(box.N) ** 3 / len(halos)) - 1.
    k, p_hm, modes = box.power_spectrum(delta_h, second=matter)
    _, p_mm, _ = box.power_spectrum(matter)
    good = np.isfinite(p_mm)                       # the first bin holds k = 0 only: empty
    k, p_hm, p_mm, modes = k[good], p_hm[good], p_mm[good], modes[good]
    low = slice(0, 4)
    bias = float(np.sum(modes[low] * p_hm[low]) / np.sum(modes[low] * p_mm[low]))
    for kk, a, b in list(zip(k, p_hm, p_mm))[:8]:
        print("  k = %.4f  P_hm = %10.2f  P_mm = %10.2f  P_hm / P_mm = %.3f" % (kk, a, b, a / b))
    print("large-scale bias of the halos above %.2e Msun: %.3f" % (halos.mass.min(), bias))
    return halos, k, p_hm, p_mm, bias


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
