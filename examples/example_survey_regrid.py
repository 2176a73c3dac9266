#!/usr/bin/env python
"""An observed cube and a galaxy sample on one grid: a box is realised and handed over the way a survey delivers it -- at half
the resolution, on (deg, deg, MHz) coordinates from pixel_array() / freq_array() -- then regridded back onto the box's grid with
interpolate_onto_grid, a halo catalogue of the same box is binned with grid_catalogue, and the two are crossed with
power_spectrum(second=), all on the GPU.  python examples/example_survey_regrid.py [nsamp]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo, analysis
from fastbox_amd.halos import HaloDistribution


def main(nsamp=64):
    np.random.seed(10)
    box = CosmoBox(cosmo=default_cosmo, box_scale=(2e3, 2e3, 2e3), nsamp=nsamp, redshift=0.8, realise_now=False)
    box.realise_density()
    N = box.N

    # The "observed" cube: 2 x 2 x 2 voxels averaged, on the mean coordinates of each pair.  freq_array() decreases along z;
    # the original coordinates must ascend, so the cube is turned round along the frequency axis.
    ang_x, ang_y = box.pixel_array()
    freqs = box.freq_array()
    coarse = np.asarray(box.delta_x).reshape(N // 2, 2, N // 2, 2, N // 2, 2).mean(axis=(1, 3, 5))
    pair = lambda c: c.reshape(-1, 2).mean(axis=1)
    obs, obs_coords = coarse[:, :, ::-1], (pair(ang_x), pair(ang_y), pair(freqs)[::-1])

    # Back onto the box: its own pixel and channel coordinates, in the box's axis order ('ij'); the new coordinates may come in
    # any order, so the decreasing freq_array() puts the channels back where the box has them.  The outermost half cell lies
    # outside the observed centres and comes back NaN.
    regridded = analysis.interpolate_onto_grid(obs, obs_coords, (ang_x, ang_y, freqs), box=box, indexing='ij')
    outside = np.isnan(np.asarray(regridded))
    delta_obs = np.nan_to_num(np.asarray(regridded))

    # A halo catalogue of the same box, binned into the box's cells
    halos = HaloDistribution(box, mass_range=(1e12, 1e15), mass_bins=10)
    counts = halos.halo_count_field(box.delta_x, nbar=1e-3, bias=1.)
    cat = halos.realise_halo_catalogue(counts, scatter=True, scatter_type='uniform')
    grid, _ = analysis.grid_catalogue(cat, box=box)
    mean = len(cat) / float(N) ** 3
    delta_h = grid * (1. / mean) - 1.

    k, p_x, modes = box.power_spectrum(delta_x=delta_obs, second=delta_h)
    _, p_dd, _ = box.power_spectrum(delta_x=box.delta_x)
    print("%d^3 box observed at %d^3 and regridded: %d of %d voxels outside the observed centres; %d halos binned (%d inside)"
          % (N, N // 2, outside.sum(), outside.size, len(cat), round(float(np.asarray(grid).sum()))))
    good = modes > 0                                          # the first bin, [0, dk), holds k = 0 alone, which is left out
    for kk, a, b, m in list(zip(k[good], p_x[good], p_dd[good], modes[good]))[:8]:
        print("  k = %.4f  P_obs,h = %10.2f  P_dd = %10.2f  (%d modes)" % (kk, a, b, m))
    return k[good], p_x[good], p_dd[good]


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
