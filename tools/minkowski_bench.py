"""Measurement aid (GPU): fb_minkowski_counts on a Gaussian and on a log-normal realisation, 3-D and per channel, for nt = 25
and 256 thresholds (nu = linspace(-3, 3, nt) about the field's mean), in f32 and f64, timed with HIP events on the box's stream
(median of --reps calls after one warm-up; the cube already on the device).  A call is the threshold upload, the clearing of the
histograms, the counting kernel and the read-back of the histograms with its wait.  Its byte model is one read of the cube over
8 TB/s; the tile halos make the kernel read 1.31 (3-D) or 1.27 (per channel, nt + 1 <= 32) voxels per voxel, mostly from cache.
And the numpy statement of tests/minkowski_numpy.py at --host-size on one core.

    python tools/minkowski_bench.py [--precs f32,f64] [--sizes 256,512] [--nts 25,256] [--reps 5] [--host-size 128]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, minkowski                    # noqa: E402

PEAK = 8e12                                                                    # bytes per second (spec)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    timed(fn)
    return float(np.median([timed(fn) for _ in range(reps)]))


def make_box(N, prec):
    stream = torch.cuda.current_stream().cuda_stream
    return CosmoBox(cosmo=default_cosmo, box_scale=2. * N, nsamp=N, realise_now=False, precision=prec, rng="device", seed=3,
                    stream=stream or None)


def device(box, nts, reps):
    eng, N = box.engine, box.N
    item = np.dtype(eng.rdtype).itemsize
    gauss = box.realise_density(inplace=False)
    fields = (("gaussian", gauss), ("lognormal", box.lognormal(gauss)))
    for name, f in fields:
        f.ptr                                                                  # materialise the deferred field
        mean, sigma = minkowski.field_moments(f)
        for per_channel in (False, True):
            for nt in nts:
                t = mean + np.linspace(-3., 3., nt) * sigma
                ms = median_ms(lambda: minkowski._counts(eng, f, t, 1 if per_channel else 0), reps)
                model = 1e3 * float(N) ** 3 * item / PEAK
                yield dict(what="minkowski", prec=eng.precision, N=N, field=name, mode="per_channel" if per_channel else "3d",
                           nt=nt, ms=round(ms, 3), model_ms=round(model, 4), ratio=round(ms / model, 1),
                           gvoxel_per_s=round(float(N) ** 3 / (ms * 1e-3) / 1e9, 2))


def host(s, nt):
    from tests import minkowski_numpy as mn
    f = np.random.RandomState(1).normal(size=(s, s, s))
    t = np.linspace(-3., 3., nt)
    t0 = time.time()
    mn.counts_3d(f, t)
    t1 = time.time()
    mn.counts_per_channel(f, t)
    t2 = time.time()
    return dict(what="host", N=s, nt=nt, numpy_3d_ms=round(1e3 * (t1 - t0), 1), numpy_per_channel_ms=round(1e3 * (t2 - t1), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--nts", default="25,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-size", type=int, default=128, help="0: no host reference")
    a = ap.parse_args()
    nts = [int(x) for x in a.nts.split(",") if x]
    for prec in [x for x in a.precs.split(",") if x]:
        for N in [int(x) for x in a.sizes.split(",") if x]:
            box = make_box(N, prec)
            for row in device(box, nts, a.reps):
                print(json.dumps(row), flush=True)
            box.engine.release_idle_buffers()
            del box
            torch.cuda.empty_cache()
    if a.host_size:
        print(json.dumps(host(a.host_size, nts[0])), flush=True)


if __name__ == "__main__":
    main()
