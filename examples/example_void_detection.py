#!/usr/bin/env python
"""Void detection in a redshift-space density field (cf. the reference's examples/example_void_detection.py, plots left out).
The watershed runs on the device; ``literal=True`` then drives the reference's per-region loop in host numpy over the device
labels, the default takes the region means from one device call (voids.region_statistics).
python examples/example_void_detection.py [nsamp]"""
import sys, os
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from fastbox_amd import CosmoBox, default_cosmo
from fastbox_amd.voids import watershed, region_statistics


def main(nsamp=64, literal=False):
    np.random.seed(10)
    box = CosmoBox(cosmo=default_cosmo, box_scale=(1e3, 1e3, 1e3), nsamp=nsamp, realise_now=False)
    box.realise_density()
    box.realise_velocity()
    vel_z = box.to_real(box.velocity_k[2])
    delta_s = box.redshift_space_density(delta_x=box.delta_x, velocity_z=vel_z, sigma_nl=200., method='linear')

    print("Running watershed algorithm")
    t0 = time.time()
    region_labels = watershed(delta_s, markers=None)
    print("Watershed took %2.2f sec" % (time.time() - t0))
    if literal:
        labels = np.asarray(region_labels).astype(np.float64)
        d = np.asarray(delta_s)
        print("No. regions:", np.unique(labels).size)
        regions = np.unique(labels)
        avg_delta = np.zeros(regions.shape)
        accepted_regions = []
        for i, r in enumerate(regions):
            if i % 100 == 0:
                print("    Region", i)
            avg_delta[i] = np.mean(d[np.where(labels == r)], dtype=np.float64)
            if avg_delta[i] > -0.1:
                labels[np.where(labels == r)] = np.inf
            else:
                accepted_regions.append(r)
    else:
        st = region_statistics(region_labels, delta_s)
        regions = np.nonzero(st.count > 0)[0]
        print("No. regions:", regions.size)
        accepted_regions = regions[~(st.mean[regions] > -0.1)]
    print("No. regions kept:", len(accepted_regions))
    return np.asarray(accepted_regions, dtype=np.int64)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
