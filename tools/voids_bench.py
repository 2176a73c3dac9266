"""Measurement aid (GPU): void finding at 128^3, 256^3 and 512^3 -- median HIP-event time of the watershed (mask f <= 0), the
region statistics, the merging (threshold 0.2) and the stacking of the merged voids of 8 .. 10^5 voxels on a 31^3 grid, each
call bracketed by events on the box's stream, warm-up excluded, with a byte model for comparison; and the numpy statement
(tests/voids_numpy.py) of the same four steps at 64^3 on one host core, for scale.

    python tools/voids_bench.py [--sizes 128,256,512] [--prec f32] [--reps 5] [--host-size 64]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, voids                         # noqa: E402
from tests import voids_numpy as vn                                            # noqa: E402


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


def host(N):
    box = CosmoBox(cosmo=default_cosmo, box_scale=7.8125 * N, nsamp=N, realise_now=False, precision="f64", rng="device", seed=3)
    f = np.asarray(box.realise_density())
    t = [time.time()]
    lab, n = vn.watershed(f, vn.inside(f, threshold=0.))
    t.append(time.time())
    st = vn.region_stats(lab, n, f)
    t.append(time.time())
    mg, M = vn.merge(lab, n, st["mean"], 0.2)
    t.append(time.time())
    sm = vn.region_stats(mg, M, f)
    cat = vn.trim(sm, 8, 10 ** 5)
    cat = cat[cat > 0]
    t.append(time.time())
    vn.stack(mg, f, cat, vn.centroids(sm, box, "uniform")[cat], vn.radii(sm, box)[cat], box)
    t.append(time.time())
    d = np.diff(t) * 1e3
    print("numpy statement, N = %d, one host core: watershed %.0f ms, statistics %.0f ms, merge %.0f ms, stack (%d voids) %.0f ms"
          % (N, d[0], d[1], d[2], cat.size, d[4]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-size", type=int, default=64)
    a = ap.parse_args()
    print("void finding, %s plan, L = 7.8125 N Mpc, mask f <= 0, merge threshold 0.2; median ms of %d calls" % (a.prec, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=7.8125 * N, nsamp=N, realise_now=False, precision=a.prec, rng="device",
                       seed=3, stream=stream or None)
        d = box.realise_density()
        d.ptr
        eng = box.engine
        lab, t_ws = timed(lambda: voids._watershed(eng, d, voids.MASK_THRESHOLD, 0., None), a.reps)
        st, t_st = timed(lambda: voids.region_statistics(lab, d), a.reps)
        mg, t_mg = timed(lambda: voids.merge_regions(st, None, 0.2), a.reps)
        eng.profile_start(only=["realop"])          # in fb_merge_regions only the hooking launch is in this class
        voids.merge_regions(st, None, 0.2)
        hooks = eng.profile_stop()["realop"][1]
        sm = voids.region_statistics(mg, d)
        cat = voids.trim_by_volume(mg, 8, 10 ** 5)
        cat = cat[cat > 0]
        cen, rad = sm.centroids(box)[cat], sm.radii(box)[cat]
        _, t_sk = timed(lambda: voids.stack_voids_at(cat, mg, box, d, cen, rad), a.reps)
        b = 4 if a.prec == "f32" else 8
        n3 = N ** 3
        print("N = %d: %d regions, %d after merging, %d voids of 8 .. 10^5 voxels stacked" % (N, lab.n_labels, mg.n_labels, cat.size))
        ws = (b + 4 + 3 * 4 + 12) * n3
        print("  watershed   %8.3f ms   model: descent (read f, write parents) + count / rank / label, %.0f MB -> %.3f ms at 5 TB/s"
              " (+ 8 B per voxel and one read-back per jump round)" % (t_ws, ws / 1e6, ws / 5e12 * 1e3))
        sb = (2 * (4 + b) + 4 + b) * n3 + 11 * 8 * (lab.n_labels + 1)
        print("  statistics  %8.3f ms   model: bound, accumulate, arg-min passes over labels + field, %.0f MB -> %.3f ms at 5 TB/s;"
              " per-run atomics" % (t_st, sb / 1e6, sb / 5e12 * 1e3))
        mb = 2 * 4 * n3
        print("  merge       %8.3f ms   %d hooking rounds (the last finds nothing to join); model: per round the labels (4 B),"
              " %.0f MB -> %.3f ms at 5 TB/s" % (t_mg, hooks, mb / 1e6, mb / 5e12 * 1e3))
        print("  label 0: %d voxels (%.0f %% of the box)" % (sm.count[0], 100. * sm.count[0] / n3))
        gathers = cat.size * 31 ** 3
        print("  stack       %8.3f ms   %d voids x 31^3 points = %.2e point tests (up to 8 label + 8 field gathers each)"
              % (t_sk, cat.size, gathers))
        del box
    host(a.host_size)


if __name__ == "__main__":
    main()
