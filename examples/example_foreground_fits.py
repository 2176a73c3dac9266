#!/usr/bin/env python
"""Foreground removal by fits along the line of sight, beside the blind PCA: one cube (log-normal signal + ForegroundModel +
radiometer noise) with three channels flagged, cleaned with pca_filter (which cannot honour flags and sees every channel),
polynomial_filter (order 3 in ln T against ln nu), LSQfitting.run_fit (power law + free-free template) and gpr_filter (RBF
foreground + exponential signal kernel); P(k) of every residual over P(k) of the signal.
python examples/example_foreground_fits.py [nsamp]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, ForegroundModel, NoiseModel, filters


def main(nsamp=64):
    t0 = time.time()
    np.random.seed(10)
    N = nsamp
    box = CosmoBox(cosmo=default_cosmo, box_scale=(4e3, 4e3, 4e3), nsamp=N, redshift=0.8, realise_now=False)
    box.realise_density()
    bias, Tb = 1.3, 0.12
    signal = np.asarray(Tb * (1. + box.lognormal(box.delta_x * bias)))
    fg = ForegroundModel(box)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., smoothing_scale=4., redshift=box.redshift)
    alpha = fg.realise_spectral_index(mean_spec_idx=2.07, std_spec_idx=0.0002, smoothing_scale=15., redshift=box.redshift)
    noise = np.asarray(NoiseModel(box).realise_radiometer_noise(Tinst=18., tp=2., fov=1., Ndish=64))
    freqs = box.freq_array()
    fg_cube = np.asarray(fg.construct_cube(fg_map, alpha, freq_ref=130., redshift=box.redshift))
    # the fits in ln T need a positive sky: a smooth power-law offset lifts the faintest voxel to 10 times the noise rms
    fg_cube = fg_cube + max(0., 10. * noise.std() - fg_cube.min()) * (freqs / freqs.max()) ** -2.07
    data = signal + fg_cube + noise
    sigma = noise.reshape(-1, N).std(axis=0)                               # per channel; known from the radiometer equation

    w = np.ones(N)                                                         # 1 = good
    w[[N // 5, N // 2, N // 2 + 1]] = 0.

    residuals = {"uncleaned": data}
    residuals["pca_filter"] = np.asarray(filters.pca_filter(data, nmodes=4, box=box))
    residuals["polynomial_filter"] = np.asarray(filters.polynomial_filter(data, order=3, space="loglog", weights=w, box=box))
    resid, bsval, fit = filters.LSQfitting(box).run_fit(data, sigma=sigma, weights=w, return_filter=True)
    residuals["run_fit"] = np.asarray(resid)
    cleaned, gpr = filters.gpr_filter(data, return_filter=True, opt_messages=False, opt_num_restarts=4, box=box)
    residuals["gpr_filter"] = np.asarray(cleaned)

    k, pk_signal, _ = box.binned_power_spectrum(delta_x=signal - Tb)
    good = ~np.isnan(pk_signal)
    ratios = {}
    print("%d^3 in %.2f s; %d channels flagged; run_fit: %d lines of sight failed, median index %.3f; gpr_filter: ln L = %.6e from "
          "%d starts, %s, noise variance %.3e" % (N, time.time() - t0, int((w == 0.).sum()), fit.n_failed, np.nanmedian(bsval),
                                                   gpr.log_marginal_likelihood, gpr.n_starts, gpr.kernels, gpr.noise_variance))
    for name, cube in residuals.items():
        ratios[name] = (box.binned_power_spectrum(delta_x=cube)[1] / pk_signal)[good]
        print("  P_residual / P_signal, %-18s" % name, np.array2string(ratios[name][3:11], precision=3))
    return residuals, w, ratios


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
