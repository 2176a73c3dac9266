#!/usr/bin/env python
"""The cosmic web of a log-normal box on the GPU: the tidal tensor of the density smoothed over two cells, its eigenvalues, and
every voxel a void, sheet, filament or knot by the number of eigenvalues above lambda_th (the T-web of Hahn et al. 2007 and
Forero-Romero et al. 2009).  Prints the volume and mass fractions of the four classes over a scan of lambda_th -- one pass over
the tensor for the whole scan -- the mean density contrast of each class at the chosen threshold, and the power spectrum of the
filament mask beside that of the density itself.
python examples/example_cosmic_web.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, web


def main(nsamp=64, spacing=4., smoothing=8., amplitude=0.6, threshold=None, nscan=9):
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, redshift=0.8, realise_now=False, rng="device",
                   seed=31)
    delta = box.lognormal(box.realise_density() * amplitude)      # exp of a milder field: skewed, not degenerate
    tensor = box.tidal_tensor(delta, smoothing=smoothing)
    lam = np.array([np.asarray(e) for e in web.eigenvalues(tensor)])
    print("tidal tensor of a %d^3 log-normal box smoothed over %g Mpc: eigenvalue means %s, rms %s" % (
        nsamp, smoothing, np.round(lam.mean(axis=(1, 2, 3)), 4), np.round(lam.std(axis=(1, 2, 3)), 4)))
    if threshold is None:                                       # in units of the field: 0.3 of the eigenvalues' spread
        threshold = 0.3 * float(lam.std())

    scan_t = np.linspace(0., 2. * threshold, nscan)
    scan = web.classify(tensor, threshold=scan_t, weight=1. + delta)
    print("lambda_th   volume fraction: void  sheet  filament  knot      mass fraction: void  sheet  filament  knot")
    for j in range(nscan):
        print("  %6.3f                  %6.4f %6.4f   %6.4f %6.4f                    %6.4f %6.4f   %6.4f %6.4f" % (
            (scan_t[j],) + tuple(scan.volume_fraction[j]) + tuple(scan.mass_fraction[j])))

    cw = box.cosmic_web(delta, smoothing=smoothing, threshold=threshold, weight=1. + delta)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_delta = cw.weight_sums[0] / cw.counts[0] - 1.
    print("mean delta per class at lambda_th = %g: " % threshold
          + ", ".join("%s %.3f" % (n, d) for n, d in zip(web.CLASS_NAMES, mean_delta)))
    k, pk_fil, modes = box.power_spectrum(cw.mask("filament"))
    _, pk_delta, _ = box.power_spectrum(delta)
    print("      k      P(k) filament mask      P(k) delta")
    for b in range(0, k.size, max(1, k.size // 8)):
        print("  %6.4f   %12.5e     %12.5e" % (k[b], pk_fil[b], pk_delta[b]))
    return scan, cw, mean_delta, (k, pk_fil, pk_delta)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
