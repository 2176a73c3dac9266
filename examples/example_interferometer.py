#!/usr/bin/env python
"""What an interferometer does to a smooth-spectrum foreground: a hexagonal array observes the foreground cube of
examples/example_endtoend.py (Interferometer.observe: per channel, the cube's transverse modes weighted by the array's uv
coverage), and the cylindrical power spectrum P(k_perp, k_par) of the dirty cube is set beside that of the sky.  A baseline
of fixed length walks outward through the uv plane as the frequency rises, so a k_perp cell is sampled in some channels and
not in others: power that sat at k_par = 0 is thrown up to k_par > 0, the more the larger k_perp -- the wedge.  Printed: the
power at k_par > 0 relative to k_par = 0 per k_perp bin, and the power outside against inside the horizon line
k_par = k_perp r H / (c (1 + z)).
python examples/example_interferometer.py [nsamp]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, ForegroundModel, Interferometer
from fastbox_amd import interferometer as itf


def horizon_slope(box):
    """k_par / k_perp of a source on the horizon: r(z) H(z) / (c (1 + z))."""
    a = box.scale_factor
    r = itf._ccl.comoving_angular_distance(box.cosmo, a)
    Hz = 100. * box.cosmo['h'] * itf._ccl.h_over_h0(box.cosmo, a)              # km / s / Mpc
    return r * Hz / (itf.C_LIGHT / 1e3) * a


def summarise(box, cyl, slope):
    """Per k_perp bin: P(1 <= |m_z| <= 3) / P(k_par = 0); and the power (mean P x modes) outside over inside the horizon line."""
    kperp, kpar, power, modes = cyl
    low = np.nansum(power[:, 1:4] * modes[:, 1:4], axis=1) / np.sum(modes[:, 1:4], axis=1)
    outside = kpar > slope * kperp
    tot = np.where(np.isnan(power), 0., power * modes)
    return low / power[:, 0], np.sum(tot[outside]) / np.sum(tot[~outside])


def main(nsamp=64, n_side=6):
    t0 = time.time()
    np.random.seed(10)
    N = nsamp
    box = CosmoBox(cosmo=default_cosmo, box_scale=(1e3, 1e3, 1e3), nsamp=N, redshift=0.8, realise_now=False)
    fg = ForegroundModel(box)
    fg_map = fg.realise_foreground_amp(amp=57., beta=1.1, monopole=10., smoothing_scale=4., redshift=box.redshift)
    alpha = fg.realise_spectral_index(mean_spec_idx=2.07, std_spec_idx=0.0002, smoothing_scale=15., redshift=box.redshift)
    sky = fg.construct_cube(fg_map, alpha, freq_ref=130., redshift=box.redshift)

    # a compact hexagonal array scaled to the box: its longest baseline reaches 95 % of the uv grid's edge in the top channel
    sx, sy = itf.channel_scales(box)
    spacing = 0.95 * (0.5 * N / max(sx.max(), sy.max())) / (2 * (n_side - 1))
    inst = Interferometer(box, antennas=itf.hex_array(n_side, spacing))
    obs = inst.observe(sky, weighting="natural", return_psf=True)
    cov = obs.coverage

    kf = 2. * np.pi / box.Lx
    kperp_bins = np.array([0.5, 0.125 * N + 0.5, 0.3 * N + 0.5, 0.5 * N + 0.5]) * kf
    cyl = {"sky": box.cylindrical_power_spectrum(delta_x=sky, kperp_bins=kperp_bins),
           "dirty": box.cylindrical_power_spectrum(delta_x=obs.dirty, kperp_bins=kperp_bins)}
    slope = horizon_slope(box)
    print("%d^3 in %.2f s: %d antennas %.2f m apart, %d baselines, uv cell %.2f x %.2f wavelengths"
          % (N, time.time() - t0, 3 * n_side * n_side - 3 * n_side + 1, spacing, inst.uv_samples().shape[0], cov.du, cov.dv))
    print("sampled cells per channel: %d .. %d of %d; PSF peak %.6f" % (cov.ncell.min(), cov.ncell.max(), N * N, obs.psf[0, 0, 0]))
    print("horizon line: k_par = %.3f k_perp" % slope)
    out = {}
    for name in ("sky", "dirty"):
        ratio, out_in = summarise(box, cyl[name], slope)
        out[name] = (ratio, out_in)
        print("%-6s P(|m_z| = 1..3) / P(k_par = 0) per k_perp bin:" % name, " ".join("%.3e" % v for v in ratio),
              "  power outside / inside the horizon line: %.3e" % out_in)
    return cyl, out, obs


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
