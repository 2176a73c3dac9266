"""Measurement aid (GPU): CosmoBox.power_spectrum at 128^3, 256^3, 512^3 in f32 and f64, auto and cross, for mode='1d',
mode='2d' (Nmu = 5) and poles=[0, 2, 4] with the default edges -- median over calls of the HIP-event time between an event
recorded before the call and one recorded after it on the box's stream (warm-up excluded; the call ends in a synchronise of
that stream, so the region is fenced), per-kernel-class HIP-event times (Engine.profile_start / _stop) of the transforms and of
the binning (k_pk_bin + k_bin_finish), the binning's share of 8 TB/s for one read of each half spectrum, and the host numpy
statement of the definition (tests/pk_numpy.py) on one core for comparison.  For per-launch times run one size per
`rocprofv3 --kernel-trace --stats` run.

    python tools/power_bench.py [--sizes 128,256,512] [--precs f32,f64] [--reps 20] [--host-sizes 128,256]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, hostgeom                      # noqa: E402

FORMS = {"1d": dict(mode="1d"), "2d": dict(mode="2d", Nmu=5), "poles": dict(mode="1d", poles=[0, 2, 4])}


def half_bytes(N, prec):
    """One read of a stored half spectrum: N x N rows of N/2 + 1 complex values (padding and spare rows are not read)."""
    b = 4 if prec == "f32" else 8
    return N * N * (N // 2 + 1) * 2 * b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-sizes", default="128,256")
    a = ap.parse_args()
    host_sizes = [int(x) for x in a.host_sizes.split(",") if x]
    for N in [int(x) for x in a.sizes.split(",")]:
        for prec in a.precs.split(","):
            stream = torch.cuda.current_stream().cuda_stream
            box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec, rng="device",
                           seed=3, stream=stream or None)
            d1 = box.realise_density(inplace=False)
            d2 = box.realise_density(inplace=False)
            eng = box.engine
            for cross in (False, True):
                for name, kw in FORMS.items():
                    args = dict(delta_x=d1, second=d2 if cross else None, **kw)
                    for _ in range(3):                         # warm-up: code objects, pool buffers, the geometry sums
                        box.power_spectrum(**args)
                    eng.sync()
                    times = []
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        box.power_spectrum(**args)             # ends in a synchronise of the stream
                        e1.record()
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1) * 1e-3)
                    eng.profile_start(only=("fft_strided", "fft_contig", "bin"))
                    for _ in range(a.reps):
                        box.power_spectrum(**args)
                    prof = eng.profile_stop()
                    med = float(np.median(times))
                    nf = 2 if cross else 1
                    fft = (prof["fft_strided"][0] + prof["fft_contig"][0]) * 1e-3 / a.reps
                    binning = prof["bin"][0] * 1e-3 / a.reps
                    nbytes = nf * half_bytes(N, prec)
                    print("N=%d %s %-5s %-5s: call median %7.3f ms (min %7.3f, max %7.3f; %d calls); r2c %7.3f ms; binning "
                          "%7.3f ms (%d launches per call), %6.1f MB read -> %5.1f%% of 8 TB/s"
                          % (N, prec, "cross" if cross else "auto", name, med * 1e3, min(times) * 1e3, max(times) * 1e3,
                             a.reps, fft * 1e3, binning * 1e3, prof["bin"][1] // a.reps, nbytes / 1e6,
                             100. * nbytes / binning / 8e12))
                    sys.stdout.flush()
            if N in host_sizes and prec == "f64":
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import pk_numpy as pk
                h1, h2 = np.asarray(d1), np.asarray(d2)
                edges = hostgeom.power_edges((1e3,) * 3, N)
                for cross in (False, True):
                    t0 = time.perf_counter()
                    pk.power_sums(h1, h2 if cross else None, (1e3,) * 3, edges, Nmu=5, lmax=0)
                    print("    host numpy statement N=%d %s 2d (float64, one core): %.2f s"
                          % (N, "cross" if cross else "auto", time.perf_counter() - t0))
                del h1, h2
            del box, d1, d2
            sys.stdout.flush()


if __name__ == "__main__":
    main()
