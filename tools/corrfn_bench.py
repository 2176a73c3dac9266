"""Measurement aid (GPU): CosmoBox.correlation_function at 128^3, 256^3, 512^3 -- median over calls of the HIP-event time
between an event recorded before the call and one recorded after it on the box's stream (warm-up excluded; the call ends in
a synchronise of that stream, so the region is fenced), the host wall-clock time of the same calls, per-kernel-class HIP-event
times (Engine.profile_start / _stop) with each class's bytes by the model below and its fraction of 8 TB/s, and the host numpy
statement of the definition (tests/corrfn_numpy.py) on one core for comparison.  For per-launch times run one size per
`rocprofv3 --kernel-trace --stats` run (launches of different sizes can share a grid size).

    python tools/corrfn_bench.py [--sizes 128,256,512] [--prec f32] [--reps 10] [--bins notebook|default] [--no-host]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo                                # noqa: E402


def edges_for(box, bins):
    if bins == "notebook":                                     # End-to-end notebooks, step (6): dr=2, rmin=20, rmax=200
        return dict(dr=2., rmin=20., rmax=200.)
    return {}                                                  # dr = cell, rmax = L/2: every cell is binned


def model_bytes(N, prec, visited):
    """Bytes per call by kernel class: r2c ~2.5 sweeps of a real field, product 1 read + 1 write of the half spectrum,
    c2r ~3 sweeps, binning = the cells read (npairs summed: each binned cell is read once)."""
    b = 4 if prec == "f32" else 8
    real = N ** 3 * b
    half = N * (N + 1) * (((N // 2 + 1) + 15) // 16 * 16) * 2 * b
    return {"r2c": 2.5 * real, "product": 2. * half, "c2r": 3. * real, "binning": visited * b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bins", default="notebook")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    for N in [int(x) for x in a.sizes.split(",")]:
        # the box runs on torch's current stream, so that torch's HIP events bracket its work on that stream
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=a.prec, rng="device", seed=3,
                       stream=stream or None)
        dx = box.realise_density()
        kw = edges_for(box, a.bins)
        kw["poles"] = [0, 2, 4]
        for _ in range(3):                                     # warm-up: code objects, pool buffers, the geometry sums
            r, xi, npairs = box.correlation_function(delta_x=dx, **kw)
        eng = box.engine
        eng.sync()
        times, walls = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            box.correlation_function(delta_x=dx, **kw)        # ends in a synchronise of the stream
            e1.record()
            e1.synchronize()
            walls.append(time.perf_counter() - t0)
            times.append(e0.elapsed_time(e1) * 1e-3)
        eng.profile_start(only=("fft_strided", "fft_contig", "filter", "bin"))
        for _ in range(a.reps):
            box.correlation_function(delta_x=dx, **kw)
        prof = eng.profile_stop()
        med = float(np.median(times))
        visited = float(np.sum(npairs))
        mb = model_bytes(N, a.prec, visited)
        print("N=%d %s bins=%s nbins=%d: HIP events median %.3f ms per call (min %.3f, max %.3f; %d calls), host wall clock "
              "median %.3f ms; cells binned %.0f (%.1f%% of the grid)"
              % (N, a.prec, a.bins, npairs.size, med * 1e3, min(times) * 1e3, max(times) * 1e3, a.reps,
                 float(np.median(walls)) * 1e3, visited, 100. * visited / N ** 3))
        per = {"fft (r2c + c2r)": (prof["fft_strided"][0] + prof["fft_contig"][0], prof["fft_strided"][1] + prof["fft_contig"][1],
                                   mb["r2c"] + mb["c2r"]),
               "product (k_cross_power)": prof["filter"] + (mb["product"],),
               "binning (k_sep_bin + k_bin_finish)": prof["bin"] + (mb["binning"],)}
        for k, (ms, cnt, nbytes) in per.items():
            t = ms * 1e-3 / a.reps
            print("    HIP events %-36s %8.3f ms per call (%2d launches), model %8.1f MB -> %5.1f%% of 8 TB/s"
                  % (k, t * 1e3, cnt // a.reps, nbytes / 1e6, 100. * nbytes / t / 8e12))
        tot = sum(mb.values())
        print("    model bytes per call: total %.1f MB -> %.1f%% of 8 TB/s at the median call time" % (tot / 1e6, 100. * tot / med / 8e12))
        if not a.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import corrfn_numpy as cf
            h = np.asarray(dx)
            edges = np.arange(20., 200. + 1., 2.) if a.bins == "notebook" else np.arange(0., 500. + 0.5e3 / N, 1e3 / N)
            t0 = time.perf_counter()
            cf.correlation_function(h, None, (1e3,) * 3, edges, poles=(0, 2, 4))
            print("    host numpy oracle (float64, one core): %.2f s" % (time.perf_counter() - t0))
            del h
        del box, dx
        sys.stdout.flush()


if __name__ == "__main__":
    main()
