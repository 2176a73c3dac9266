"""Measurement aid (GPU): the pieces of CosmoBox.cylindrical_power_spectrum and CosmoBox.angular_power_spectrum at 256^3 and
512^3 in f32 and f64 with the default edges -- the r2c; the cylindrical binning (fb_bin_power_cyl: k_cyl_rows + k_cyl_finish)
beside fb_bin_power_kmu (mode '2d', Nmu = 5) on the same half spectrum in the same run; the transverse transform
(fb_real_to_complex + fb_fft_transverse); the Gram (fb_transverse_gram: k_maps_gram + k_maps_finish) beside
fb_channel_covariance on the same cube in the same run.  Two numbers per piece: the median over calls of the HIP-event time
between events recorded around the call on the box's stream (the binning and Gram entries end in a synchronise, and their host
work -- tables, the record -- is inside), and the per-kernel-class HIP-event time of its kernels alone (Engine.profile_start /
_stop).  Models: the binning reads each half spectrum once (share of 8 TB/s); the Gram is 4 N^4 flops whatever the number of
bins, the covariance 2 N^4 (rate in TFLOP/s).

    python tools/cylindrical_bench.py [--sizes 256,512] [--precs f32,f64] [--reps 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, hostgeom, _lib               # noqa: E402


def half_bytes(N, prec):
    """One read of a stored half spectrum: N x N rows of N/2 + 1 complex values (padding and spare rows are not read)."""
    return N * N * (N // 2 + 1) * 2 * (4 if prec == "f32" else 8)


def timed(eng, fn, reps, classes):
    """(median event seconds per call, kernel-class seconds per call, launches per call) of fn()."""
    for _ in range(2):
        fn()
    eng.sync()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    eng.profile_start(only=classes)
    for _ in range(reps):
        fn()
    eng.sync()
    prof = eng.profile_stop()
    return (float(np.median(times)), sum(prof[c][0] for c in classes) * 1e-3 / reps, sum(prof[c][1] for c in classes) // reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    P = _lib.P_double
    for N in [int(x) for x in a.sizes.split(",")]:
        for prec in a.precs.split(","):
            stream = torch.cuda.current_stream().cuda_stream
            L = (1e3, 1e3, 1e3)
            box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec, rng="device",
                           seed=3, stream=stream or None)
            eng = box.engine
            d1 = box._as_real(box.realise_density(inplace=False))
            d2 = box._as_real(box.realise_density(inplace=False))
            tag = "N=%d %s" % (N, prec)
            # ---- r2c, then the two binnings on the same spectra
            h1, h2 = eng.empty("half"), eng.empty("half")
            r2c = lambda: _lib.call("fb_fft_r2c", eng._plan, d1.ptr, h1.ptr, 0, eng.stream)
            ev, ker, nl = timed(eng, r2c, a.reps, ("fft_strided", "fft_contig"))
            print("%s r2c: call %7.3f ms, kernels %7.3f ms" % (tag, ev * 1e3, ker * 1e3))
            _lib.call("fb_fft_r2c", eng._plan, d2.ptr, h2.ptr, 0, eng.stream)
            pe, qe = hostgeom.cyl_edges(L, N)
            ke = hostgeom.power_edges(L, N)
            nperp, npar, nk, nmu = pe.size - 1, qe.size - 1, ke.size - 1, 5
            out_c, out_k = np.zeros(4 * nperp * npar), np.zeros(4 * nk * nmu)
            for cross in (False, True):
                second = h2.ptr if cross else None
                cyl = lambda: _lib.call("fb_bin_power_cyl", eng._plan, h1.ptr, second, pe.ctypes.data_as(P), nperp,
                                        qe.ctypes.data_as(P), npar, out_c.ctypes.data_as(P), eng.stream)
                kmu = lambda: _lib.call("fb_bin_power_kmu", eng._plan, h1.ptr, second, ke.ctypes.data_as(P), nk, nmu, 0,
                                        out_k.ctypes.data_as(P), eng.stream)
                nbytes = (2 if cross else 1) * half_bytes(N, prec)
                rates = []
                for name, fn in (("cylindrical %dx%d" % (nperp, npar), cyl), ("(k, mu) %dx%d" % (nk, nmu), kmu)):
                    ev, ker, nl = timed(eng, fn, a.reps, ("bin",))
                    rates.append(nbytes / ker)
                    print("%s binning %-5s %-20s: call %7.3f ms, kernels %7.3f ms (%d launches), %6.1f MB read -> %5.1f%% of "
                          "8 TB/s" % (tag, "cross" if cross else "auto", name, ev * 1e3, ker * 1e3, nl, nbytes / 1e6,
                                      100. * nbytes / ker / 8e12))
                print("%s binning %-5s: cylindrical reaches %.2f x the bytes/s of (k, mu)"
                      % (tag, "cross" if cross else "auto", rates[0] / rates[1]))
            del h1, h2
            # ---- the transverse transform, then the Gram beside the channel covariance
            if N <= hostgeom.MAPS_MAX_N:
                f1, f2 = eng.empty("full"), eng.empty("full")

                def transverse(d=d1, f=f1):
                    _lib.call("fb_real_to_complex", eng._plan, d.ptr, f.ptr, eng.stream)
                    _lib.call("fb_fft_transverse", eng._plan, f.ptr, -1, eng.stream)
                ev, ker, nl = timed(eng, transverse, a.reps, ("fft_strided", "fft_contig", "layout"))
                print("%s transverse transform: call %7.3f ms, kernels %7.3f ms" % (tag, ev * 1e3, ker * 1e3))
                transverse(d2, f2)
                me = hostgeom.maps_edges(L, N)
                nb = me.size - 1
                rec = np.zeros(2 * nb)
                mean_dev, cov_dev = eng._alloc_bytes(N * 8), eng._alloc_bytes(N * N * 8)
                _lib.call("fb_channel_means", eng._plan, d1.ptr, mean_dev.ptr, eng.stream)
                cov = lambda: _lib.call("fb_channel_covariance", eng._plan, d1.ptr, mean_dev.ptr, cov_dev.ptr, eng.stream)
                ev, ker, nl = timed(eng, cov, a.reps, ("pca",))
                cov_rate = 2. * float(N) ** 4 / ker
                print("%s channel covariance       : call %7.3f ms, kernels %7.3f ms, 2 N^4 flops -> %6.2f TFLOP/s"
                      % (tag, ev * 1e3, ker * 1e3, cov_rate / 1e12))
                cl_dev = eng._alloc_bytes(nb * N * N * 8)
                for cross in (False, True):
                    work = eng._alloc_bytes(_lib.load().fb_transverse_gram_work_bytes(eng._plan, nb, 1 if cross else 0))
                    gram = lambda: _lib.call("fb_transverse_gram", eng._plan, f1.ptr, f2.ptr if cross else None,
                                             me.ctypes.data_as(P), nb, cl_dev.ptr, work.ptr, rec.ctypes.data_as(P), eng.stream)
                    ev, ker, nl = timed(eng, gram, a.reps, ("pca",))
                    rate = 4. * float(N) ** 4 / ker
                    print("%s Gram %-5s %3d bins       : call %7.3f ms, kernels %7.3f ms, 4 N^4 flops -> %6.2f TFLOP/s, %.2f x the "
                          "covariance's rate; work %.0f MB" % (tag, "cross" if cross else "auto", nb, ev * 1e3, ker * 1e3,
                                                                rate / 1e12, rate / cov_rate, work.nbytes / 1e6))
                    del work
                del f1, f2, cl_dev
            del box, d1, d2
            sys.stdout.flush()


if __name__ == "__main__":
    main()
