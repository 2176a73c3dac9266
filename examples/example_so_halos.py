#!/usr/bin/env python
"""Spherical-overdensity masses of the halos of a COLA run, all on the GPU: a COLA particle-mesh realisation that keeps its
particles, friends-of-friends halos (b = 0.2, 20 members or more), then around every friends-of-friends centre the radial
profile of all particles, R_200 and M_200 against the mean density, and the members, centre of mass and velocity dispersion
inside R_200.  Printed: the cumulative mass function of M_200 beside that of the friends-of-friends masses, and the stacked
density profile of the halos in units of R_200.  python examples/example_so_halos.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo


def main(nsamp=128, spacing=2., delta=200.):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, realise_now=False, rng="device", seed=10)

    # COLA particles with their velocities, and their friends-of-friends halos
    _, particles = box.realise_density_cola(redshift=0., keep_velocities=False, return_particles=True)
    fof = box.find_halos(particles, linking_length=0.2, nmin=20)

    # Spherical-overdensity radii and masses around the friends-of-friends centres
    so = box.spherical_overdensity(fof, particles, delta=delta, reference='mean', rmin=0.125 * spacing)
    good = so.status == 0
    print("%d particles -> %d friends-of-friends halos; %d have an R_%g (status 1: %d, status 2: %d); rho_ref = %.3e Msun / Mpc^3"
          % (len(particles), len(fof), good.sum(), delta, np.sum(so.status == 1), np.sum(so.status == 2), so.rho_ref))
    for h in np.nonzero(good)[0][:5]:
        print("  FoF %5d members, M = %.3e | R_%g = %.3f Mpc, M_%g = %.3e Msun, %5d members, sigma_v = %4.0f km/s"
              % (fof.count[h], fof.mass[h], delta, so.radius[h], delta, so.mass[h], so.count[h], so.sigma_v[h]))

    # Cumulative mass functions n(> M) per Mpc^3
    volume = box.Lx * box.Ly * box.Lz
    masses = np.geomspace(fof.mass.min(), fof.mass.max(), 8)
    n_fof = np.array([np.sum(fof.mass >= m) for m in masses]) / volume
    n_so = np.array([np.sum(so.mass[good] >= m) for m in masses]) / volume
    for m, a, b in zip(masses, n_fof, n_so):
        print("  M > %.3e Msun: n_FoF = %.3e, n_SO = %.3e per Mpc^3" % (m, a, b))

    # Stacked density profile in units of R_200: every halo's shell densities, interpolated in log r onto x = r / R
    x = np.geomspace(0.3, 1.5, 8)
    prof = so.profiles
    stack = np.zeros_like(x)
    used = 0
    for h in np.nonzero(good)[0]:
        r = prof.r / so.radius[h]
        if r[0] <= x[0] and r[-1] >= x[-1]:
            stack += np.interp(np.log(x), np.log(r), prof.density[h])
            used += 1
    stack /= max(used, 1) * so.rho_ref
    print("stacked rho(r) / rho_ref of %d halos:" % used)
    for xx, s in zip(x, stack):
        print("  r / R = %.3f: %10.2f" % (xx, s))
    return fof, so, masses, n_fof, n_so, x, stack, used


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
