"""Measurement aid (GPU): the halo tracers at 256^3 and 512^3 for about one halo per voxel -- median over calls of the HIP-event
time of halo_count_field (rng='device'), realise_halo_catalogue (scatter on the device; the call includes its one read-back
of the halo total) and paint_catalogue (ngp, cic, tsc, no compensation; tsc compensated), bracketed by events on the box's
stream, warm-up excluded, with a byte model for comparison.  nbar = 1/voxel_vol, bias 1, cells of 7.8 Mpc (L = 7.8125 N Mpc): about one
halo per voxel (few voxels of negative lam are clipped to 0).

    python tools/halos_bench.py [--sizes 256,512] [--prec f32] [--reps 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo                                # noqa: E402
from fastbox_amd.halos import HaloDistribution                                 # noqa: E402


def timed(fn, reps):
    out, ts = None, []
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return out, float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print("halo tracers, %s plan, nbar = 1/voxel_vol, bias 1, L = 7.8125 N Mpc; median ms of %d calls" % (a.prec, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream
        L = 7.8125 * N
        box = CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=a.prec, rng="device", seed=3,
                       stream=stream or None)
        dx = box.realise_density()
        hd = HaloDistribution(box, (1e12, 1e15), 10)
        vv = L ** 3 / N ** 3.
        c, t_counts = timed(lambda: hd.halo_count_field(dx, 1. / vv, 1.), a.reps)
        cat, t_cat = timed(lambda: hd.realise_halo_catalogue(c, scatter=True), a.reps)
        nh = len(cat)
        res = {}
        for win, comp in (("ngp", False), ("cic", False), ("tsc", False), ("tsc", True)):
            _, res[(win, comp)] = timed(lambda: box.paint_catalogue(cat, window=win, compensated=comp), a.reps)
        b = 4 if a.prec == "f32" else 8
        n3 = N ** 3
        print("N = %d: %d halos (%.3f per voxel)" % (N, nh, nh / float(n3)))
        print("  counts      %8.3f ms   model: read delta + write counts = %.0f MB -> %.3f ms at 5 TB/s"
              % (t_counts, 2 * b * n3 / 1e6, 2 * b * n3 / 5e12 * 1e3))
        cat_bytes = 3 * b * n3 + 24 * nh
        print("  catalogue   %8.3f ms   model: 3 reads of the counts + 24 B/halo = %.0f MB -> %.3f ms at 5 TB/s"
              % (t_cat, cat_bytes / 1e6, cat_bytes / 5e12 * 1e3))
        acc = (16 if a.prec == "f64" else 8) * n3
        for (win, comp), t in res.items():
            nodes = {"ngp": 1, "cic": 8, "tsc": 27}[win]
            print("  paint %-3s%s %8.3f ms   %d x %d fixed-point atomic adds (%.1f G/s); accumulator %.0f MB"
                  % (win, " comp" if comp else "     ", t, nh, nodes * (2 if a.prec == "f64" else 1),
                     nh * nodes * (2 if a.prec == "f64" else 1) / (t * 1e-3) / 1e9, acc / 1e6))
        del box


if __name__ == "__main__":
    main()
