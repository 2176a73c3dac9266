#!/usr/bin/env python
"""The delay spectrum of a flagged cube without filling its holes: a foreground-free cube (signal + noise) loses 10 % of its
channels in every line of sight and 1 % of its voxels at random (NaN, as RFI flagging leaves them).  Least-squares spectral
analysis (inpaint.lssa_delay_spectrum) fits every delay mode to the unflagged channels of each line of sight and averages the
decorrelated power over the lines of sight; its spectrum of the flagged cube is printed beside that of the unflagged cube and
of the cube in-painted by a constrained realisation (inpaint.inpaint_cube) -- the standard check on an in-painting prior.
python examples/example_lssa.py [nsamp]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, NoiseModel, inpaint


def main(nsamp=64):
    t0 = time.time()
    np.random.seed(12)
    N = nsamp
    box = CosmoBox(cosmo=default_cosmo, box_scale=(4e3, 4e3, 4e3), nsamp=N, redshift=0.8, realise_now=False)
    box.realise_density()
    bias, Tb = 1.3, 0.12
    signal_cube = Tb * (1. + box.lognormal(box.delta_x * bias))
    noise = NoiseModel(box).realise_radiometer_noise(Tinst=18., tp=2., fov=1., Ndish=64)
    data = np.asarray(signal_cube + noise)
    noise_var = np.asarray(noise).reshape(-1, N).var(axis=0)
    chan_mean = data.reshape(-1, N).mean(axis=0)
    data = data - chan_mean                                             # the spectrum of the fluctuations

    # flags: 1 = good.  10 % of the channels everywhere, 1 % of the voxels at random
    w = np.ones((N, N, N))
    w[:, :, np.random.choice(N, size=max(1, N // 10), replace=False)] = 0.
    w[np.random.uniform(size=w.shape) < 0.01] = 0.
    flagged = np.where(w == 0., np.nan, data)

    taper = np.hanning(N + 2)[1:-1]                                     # without the zeros at the ends
    full = inpaint.lssa_delay_spectrum(data, np.ones(N), N=noise_var, taper=taper, box=box)
    holes = inpaint.lssa_delay_spectrum(flagged, w, N=noise_var, taper=taper, box=box)
    # the prior of the in-painting: the frequency-frequency covariance of the unflagged channels' neighbours, here simply
    # that of the cube with its holes set to zero, minus the noise
    x = np.where(w == 0., 0., data).reshape(-1, N)
    S = np.cov(x.T) - np.diag(noise_var)
    lam, V = np.linalg.eigh(S)
    S = (V * np.maximum(lam, 1e-12 * lam.max())) @ V.T
    painted = inpaint.inpaint_cube(flagged, w, S, noise_var, box=box, tol=1e-8, cg_maxiter=500)
    filled = inpaint.lssa_delay_spectrum(painted, np.ones(N), N=noise_var, taper=taper, box=box)

    order = np.argsort(full.tau)
    print("%d^3 in %.2f s; %d of %d channels flagged everywhere, %d lines of sight" % (
        N, time.time() - t0, int((w.reshape(-1, N) == 0.).all(axis=0).sum()), N, holes.n_los))
    print("   tau [ns]    unflagged        LSSA of the flagged cube    in-painted")
    for n in order[::max(1, N // 16)]:
        print("  %9.2f   %.4e   %.4e +- %.1e   %.4e" % (full.tau[n], full.ps_mean[n], holes.ps_mean[n], holes.ps_stderr[n],
                                                      filled.ps_mean[n]))
    return full, holes, filled, w


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
