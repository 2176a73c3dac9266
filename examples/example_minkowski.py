#!/usr/bin/env python
"""Minkowski functionals of excursion sets on the GPU: a Gaussian and a log-normal realisation of one box, both smoothed with a
Gaussian through ``apply_transfer_fn``, their volume, surface, mean-curvature and Euler-characteristic densities V0 .. V3
against the threshold nu beside what a Gaussian field of the same spectral moments gives -- the log-normal field departs from
it, which no power spectrum shows -- and then the per-channel Euler characteristic of a data cube with foregrounds before and
after ``pca_filter``, beside the signal's own: what the foregrounds and the cleaning step do to the topology of each channel.
python examples/example_minkowski.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, ForegroundModel, filters, minkowski


def main(nsamp=128, spacing=4., smoothing=8., amplitude=0.6, nmodes=3, nnu=13):
    np.random.seed(4)                                      # the foreground maps draw from numpy's stream
    box = CosmoBox(cosmo=default_cosmo, box_scale=spacing * nsamp, nsamp=nsamp, redshift=0.8, realise_now=False, rng="device",
                   seed=31)
    gauss = box.realise_density()
    lognormal = box.lognormal(gauss * amplitude)             # exp of a milder field: skewed, not degenerate

    def window(k_perp, k_par):
        return np.exp(-0.5 * (k_perp ** 2 + k_par ** 2) * smoothing ** 2)
    nu = np.linspace(-3., 3., nnu)
    out = {}
    for name, field in (("Gaussian", gauss), ("log-normal", lognormal)):
        smooth = box.apply_transfer_fn(box.to_k(field), window).real
        mf = box.minkowski_functionals(smooth, nu=nu)
        s0, s1 = minkowski.spectral_moments(box, smooth)
        theory = minkowski.gaussian_minkowski(nu, s0, s1)
        print("%s field smoothed over %g Mpc: sigma0 = %.4f, sigma1 = %.5f / Mpc" % (name, smoothing, s0, s1))
        print("     nu      V0  (Gauss)     V1 x 1e3 (Gauss)     V2 x 1e5 (Gauss)     V3 x 1e7 (Gauss)")
        for j in range(nnu):
            print("  %5.2f   %6.4f (%6.4f)   %8.4f (%8.4f)   %8.4f (%8.4f)   %8.4f (%8.4f)" % (
                nu[j], mf.v0[j], theory[0][j], 1e3 * mf.v1[j], 1e3 * theory[1][j], 1e5 * mf.v2[j], 1e5 * theory[2][j],
                1e7 * mf.v3[j], 1e7 * theory[3][j]))
        out[name] = (mf, theory)

    # a data cube: the signal under smooth-spectrum foregrounds; per-channel Euler characteristic at nu = 0 of each channel
    signal = 0.1 * (1. + box.lognormal(gauss))
    fg = ForegroundModel(box)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., smoothing_scale=0.5, redshift=box.redshift)
    alpha = fg.realise_spectral_index(mean_spec_idx=2.07, std_spec_idx=0.0002, smoothing_scale=2., redshift=box.redshift)
    data = signal + fg.construct_cube(fg_map, alpha, freq_ref=130., redshift=box.redshift)
    cleaned = filters.pca_filter(data, nmodes=nmodes)
    v2 = [minkowski.minkowski_functionals(c, nu=[0.], per_channel=True).v2[:, 0] for c in (signal, data, cleaned)]
    print("per-channel Euler characteristic density v2 x 1e4 at nu = 0: signal, signal + foregrounds, after pca_filter(nmodes=%d)" % nmodes)
    for c in range(0, nsamp, max(1, nsamp // 8)):
        print("   channel %4d   %9.4f   %9.4f   %9.4f" % (c, 1e4 * v2[0][c], 1e4 * v2[1][c], 1e4 * v2[2][c]))
    return nu, out["Gaussian"], out["log-normal"], np.array(v2)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
