#!/usr/bin/env python
"""What PCA cleaning does in the plane the instrument lives in: the data cube of examples/example_endtoend.py (signal +
foregrounds + noise) before and after filters.pca_filter, as the cylindrical power spectrum P(k_perp, k_par) beside that of the
signal alone, and as the channel correlation coefficient C_b(nu, nu') / sqrt(C_b(nu, nu) C_b(nu', nu')) of the multi-frequency
angular power spectrum: foregrounds tie every pair of channels together (coefficient ~ 1, power piled up at low k_par), the
cleaned cube is left with the signal's and the noise's short-range correlation.
python examples/example_cylindrical_power.py [nsamp]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, ForegroundModel, NoiseModel, filters


def channel_coefficients(cl):
    """C_b(nu, nu') / sqrt(C_b(nu, nu) C_b(nu', nu')) per bin."""
    dg = np.sqrt(np.einsum("bii->bi", cl))
    return cl / (dg[:, :, None] * dg[:, None, :])


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
    cleaned = filters.pca_filter(data_cube, nmodes=4, box=box)

    # coarse cells: four k_perp bins, and k_par = 0 (where a smooth spectrum lives), the next three |m_z|, the rest
    kf = 2. * np.pi / box.Lx
    kperp_bins = np.array([0.5, 2.5, 6.5, 14.5, 0.5 * N + 0.5]) * kf
    kpar_bins = np.array([-0.5, 0.5, 3.5, 0.5 * N + 0.5]) * kf
    cyl = {}
    for name, cube in (("signal", signal_cube - Tb), ("contaminated", data_cube), ("cleaned", cleaned)):
        cyl[name] = box.cylindrical_power_spectrum(delta_x=cube, kperp_bins=kperp_bins, kpar_bins=kpar_bins)
    maps = {}
    for name, cube in (("contaminated", data_cube), ("cleaned", cleaned)):
        maps[name] = box.angular_power_spectrum(delta_x=cube, kperp_bins=kperp_bins)
    print("%d^3 in %.2f s" % (N, time.time() - t0))
    kperp, kpar = cyl["signal"][0], cyl["signal"][1]
    print("k_perp [1/Mpc] per row:", np.round(kperp[:, 0], 4), " k_par [1/Mpc] per column:", np.round(kpar[0], 4))
    for name in ("signal", "contaminated", "cleaned"):
        print("P(k_perp, k_par) [mK^2 Mpc^3], %s:" % name)
        for row in cyl[name][2]:
            print("   ", " ".join("%11.4e" % v for v in row))
    off = ~np.eye(N, dtype=bool)
    for name in ("contaminated", "cleaned"):
        r = channel_coefficients(maps[name][1])
        print("channel correlation coefficient, %-12s: mean over nu != nu' per k_perp bin" % name,
              np.round([np.mean(x[off]) for x in r], 4), " neighbours |nu - nu'| = 1:",
              np.round([np.mean(np.diagonal(x, 1)) for x in r], 4))
    return cyl, maps


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
