#!/usr/bin/env python
"""Halos on a Gaussian box and their spectra (cf. the reference's examples/example_halos.py): Poisson halo counts, a halo
catalogue, the catalogue painted onto the mesh (nbodykit's to_mesh(window='tsc', compensated=True) in the reference), then
the halo-halo, matter-matter and halo-matter power spectra, all on the GPU.  The halo-matter spectrum comes from the auto
spectra: P_hd = (P(h + d) - P(h) - P(d)) / 2.  python examples/example_halos.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo
from fastbox_amd.halos import HaloDistribution


def main(nsamp=64):
    np.random.seed(10)
    box = CosmoBox(cosmo=default_cosmo, box_scale=(2e3, 2e3, 2e3), nsamp=nsamp, realise_now=False)
    box.realise_density()

    # Create halo distribution
    halos = HaloDistribution(box, mass_range=(1e12, 1e15), mass_bins=10)
    Nhalos = halos.halo_count_field(box.delta_x, nbar=1e-3, bias=1.)
    halo_cat = halos.realise_halo_catalogue(Nhalos, scatter=True, scatter_type='uniform')

    # Project catalogue onto mesh; halo overdensity (the painted counts conserve the number of halos)
    mesh = box.paint_catalogue(halo_cat, window='tsc', compensated=True)
    mean = len(halo_cat) / float(box.N) ** 3
    delta_h = mesh * (1. / mean) - 1.

    # Power spectra
    k, p_hh, _ = box.binned_power_spectrum(delta_x=delta_h)
    _, p_dd, _ = box.binned_power_spectrum(delta_x=box.delta_x)
    _, p_sum, _ = box.binned_power_spectrum(delta_x=delta_h + box.delta_x)
    p_hd = 0.5 * (p_sum - p_hh - p_dd)

    print("%d halos on a %d^3 box (%.3f per voxel)" % (len(halo_cat), box.N, mean))
    good = ~np.isnan(p_dd)
    for kk, a, b, c in list(zip(k[good], p_hh[good], p_dd[good], p_hd[good]))[:8]:
        print("  k = %.4f  P_hh = %10.2f  P_dd = %10.2f  P_hd = %10.2f" % (kk, a, b, c))
    return k, p_hh, p_dd, p_hd, len(halo_cat)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
