#!/usr/bin/env python
"""Density-field (BAO) reconstruction of a COLA run, all on the GPU: a linear field, its COLA particle-mesh evolution to z = 0
keeping the particles, then ``reconstruct`` -- the smoothed Zel'dovich displacement of the evolved density, the particles and a
set of randoms moved back by it, and the difference of the two painted sets.  Printed: the cross-correlation coefficient r(k)
with the linear field before and after, through ``power_spectrum(second=)``, and xi(r) of the two fields; then the
Landy-Szalay xi(r) of a subsample of the particles moved by the displacement of the full density (``delta=``: the
displacement may come from any mesh on the box's grid, a cleaned intensity map for instance).
python examples/example_reconstruction.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, recon


def coefficient(box, a, b, kbins):
    """r(k) = P_ab / sqrt(P_aa P_bb)"""
    k, pab, _ = box.power_spectrum(a, second=b, kbins=kbins)
    paa, pbb = box.power_spectrum(a, kbins=kbins)[1], box.power_spectrum(b, kbins=kbins)[1]
    return k, pab / np.sqrt(paa * pbb)


def main(nsamp=128, spacing=8., smoothing=15., nbins=8, subsample=8192):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, realise_now=False, rng="device", seed=21)

    # the linear field at z = 0 and its COLA evolution
    linear = box.realise_density(linear=True, redshift=0., inplace=False)
    evolved, particles = box.realise_density_cola(redshift=0., keep_velocities=False, delta_lin=linear, return_particles=True)

    # reconstruction of the matter field: bias 1, real space; one random on every mesh node
    rec = box.reconstruct(particles, randoms='grid', smoothing=smoothing, bias=1., f=0.)
    print(rec)

    kbins = np.linspace(0., np.pi / spacing, nbins + 1)
    k, r_before = coefficient(box, evolved, linear, kbins)
    _, r_after = coefficient(box, rec.delta_rec, linear, kbins)
    print("   k [1/Mpc]   r(k) evolved   r(k) reconstructed")
    for b in range(nbins):
        print("   %8.4f   %10.4f   %10.4f" % (k[b], r_before[b], r_after[b]))

    rbins = np.linspace(2. * spacing, 12. * spacing, 11)
    r, xi_before, _ = box.correlation_function(evolved, rbins=rbins)
    _, xi_after, _ = box.correlation_function(rec.delta_rec, rbins=rbins)
    _, xi_linear, _ = box.correlation_function(linear, rbins=rbins)

    # a catalogue moved by the displacement of another mesh: a subsample of the particles, the density of all of them
    pick = np.sort(np.random.RandomState(2).permutation(len(particles))[:subsample])
    sub = box.reconstruct(np.asarray(particles)[pick], randoms=4 * subsample, smoothing=smoothing, delta=evolved)
    _, xi_ls = recon.reconstructed_xi(box, sub, rbins)
    print("   r [Mpc]   xi linear   xi evolved   xi reconstructed   xi Landy-Szalay (%d particles)" % subsample)
    for b in range(r.size):
        print("   %7.2f   %9.5f   %9.5f   %9.5f   %9.5f" % (r[b], xi_linear[b], xi_before[b], xi_after[b], xi_ls[b]))
    return k, r_before, r_after, r, xi_before, xi_after, xi_ls


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
