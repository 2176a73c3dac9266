#!/usr/bin/env python
"""Flagged channels in the end-to-end flow: the data cube of examples/example_endtoend.py (signal + foregrounds + noise) loses a
few channels in nine of ten lines of sight and 1 % of its voxels at random (NaN, as RFI flagging leaves them); the holes are
filled either with the channel mean (analysis.replace_nan_with_channel_mean) or with a Gaussian constrained realisation
(inpaint.inpaint_cube, prior = the frequency-frequency covariance of the mean-filled cube), and both go through PCA cleaning and
P(k) beside the unflagged cube.
python examples/example_inpaint.py [nsamp]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, ForegroundModel, NoiseModel, filters, inpaint, analysis


def main(nsamp=64):
    t0 = time.time()
    np.random.seed(10)
    N = nsamp
    box = CosmoBox(cosmo=default_cosmo, box_scale=(4e3, 4e3, 4e3), nsamp=N, redshift=0.8, realise_now=False)
    box.realise_density()
    bias, Tb = 1.3, 0.12
    signal_cube = Tb * (1. + box.lognormal(box.delta_x * bias))
    fg = ForegroundModel(box)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., smoothing_scale=4., redshift=box.redshift)
    alpha = fg.realise_spectral_index(mean_spec_idx=2.07, std_spec_idx=0.0002, smoothing_scale=15., redshift=box.redshift)
    noise = NoiseModel(box).realise_radiometer_noise(Tinst=18., tp=2., fov=1., Ndish=64)
    data_cube = signal_cube + fg.construct_cube(fg_map, alpha, freq_ref=130., redshift=box.redshift) + noise
    noise_var = np.asarray(noise).reshape(-1, N).var(axis=0)               # per channel; known from the radiometer equation

    # flags: 1 = good.  Three channels in nine of ten lines of sight (a channel flagged everywhere has no mean to fill it
    # with: it would stay NaN in the mean-filled cube) and 1 % of the voxels
    w = np.ones((N, N, N))
    for c in (N // 5, N // 2, N // 2 + 1):
        w[:, :, c] = np.where(np.random.uniform(size=(N, N)) < 0.9, 0., 1.)
    w[np.random.uniform(size=w.shape) < 0.01] = 0.
    flagged = np.asarray(data_cube).copy()
    flagged[w == 0.] = np.nan

    mean_filled = analysis.replace_nan_with_channel_mean(flagged, box=box)
    # the prior: the frequency-frequency covariance of the mean-filled cube (foregrounds + signal + noise; a little low in the
    # flagged channels), minus the noise; the constrained realisation is drawn for the mean-subtracted cube
    x = np.asarray(mean_filled).reshape(-1, N)
    chan_mean = x.mean(axis=0)
    S = np.cov(x.T) - np.diag(noise_var)
    lam, V = np.linalg.eigh(S)
    S = (V * np.maximum(lam, 1e-12 * lam.max())) @ V.T
    centred = np.where(w == 0., np.nan, np.asarray(data_cube) - chan_mean)
    painted, info = inpaint.inpaint_cube(centred, w, S, noise_var, box=box, tol=1e-8, cg_maxiter=500, return_info=True)

    truth = np.asarray(data_cube) - chan_mean
    hole = w == 0.
    err_mean = np.sqrt(np.mean((np.asarray(mean_filled) - chan_mean - truth)[hole] ** 2))
    err_cr = np.sqrt(np.mean((np.asarray(painted) - truth)[hole] ** 2))
    k, pk_true, _ = box.binned_power_spectrum(delta_x=signal_cube - Tb)
    pks = []
    for cube in (data_cube, mean_filled, painted):
        cleaned = filters.pca_filter(cube, nmodes=4, box=box)
        pks.append(box.binned_power_spectrum(delta_x=cleaned)[1])
    good = ~np.isnan(pk_true)
    print("%d^3 in %.2f s; %d CG iterations at most, residual %.1e; rms error in the holes: channel mean %.3e, constrained "
          "realisation %.3e (noise rms %.3e)" % (N, time.time() - t0, info.max_iter_, info.residual, err_mean, err_cr,
                                                 np.sqrt(noise_var.mean())))
    for name, pk in zip(("unflagged", "channel mean", "in-painted"), pks):
        print("  P_cleaned / P_signal, %-13s" % name, np.round((pk / pk_true)[good][3:11], 3))
    return np.asarray(painted), np.asarray(mean_filled), w


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
