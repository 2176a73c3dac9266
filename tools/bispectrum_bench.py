"""Measurement aid (GPU): CosmoBox.bispectrum with 16 shells (the default edges) at 128^3, 256^3, 512^3 in f32 and 512^3 in
f64 -- median over calls of the HIP-event time between an event recorded before the call and one recorded after it on the
box's stream (warm-up excluded, the triangle counts of the edge set already formed; the call ends in a synchronise of that
stream, so the region is fenced), and per phase the median over calls of the per-kernel-class HIP-event times
(Engine.profile_start / _stop, one class per call): the shell split (k_bk_split, nb / 4 launches), the transforms (one r2c and
nb c2r), the contraction (k_bk_contract) and the finishing kernels (k_bin_finish per split launch, k_bk_finish; taken as the
difference between all launches of a class and every second one).  The contraction's share of both roofs: nb N^3 values read
once at 8 TB/s, and 2 * 16 * 16 * nb * N^3 fp64 flops on the matrix cores at 32 flops per cycle and SIMD, 1024 SIMDs, 2.4 GHz.
The host numpy statement of the definition (tests/bk_numpy.py) on one core for scale.

    python tools/bispectrum_bench.py [--cases 128:f32,256:f32,512:f32,512:f64] [--reps 20] [--host-sizes 128]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, hostgeom                      # noqa: E402

HBM = 8e12
MATRIX_FP64 = 32. * 1024 * 2.4e9


def phase(box, args, reps, only, stride):
    eng = box.engine
    out = []
    for _ in range(reps):
        eng.profile_start(only=only, stride=stride)
        box.bispectrum(**args)
        prof = eng.profile_stop()
        out.append(sum(prof[c][0] for c in only) * 1e-3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:f32,256:f32,512:f32,512:f64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-sizes", default="128")
    a = ap.parse_args()
    host_sizes = [int(x) for x in a.host_sizes.split(",") if x]
    done_host = set()
    for case in a.cases.split(","):
        N, prec = int(case.split(":")[0]), case.split(":")[1]
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec, rng="device",
                       seed=3, stream=stream or None)
        d = box.lognormal(box.realise_density(inplace=False))
        d.ptr
        eng = box.engine
        edges = hostgeom.bispectrum_edges((box.Lx, box.Ly, box.Lz), N)
        nb = edges.size - 1
        args = dict(delta_x=d, kbins=edges)
        t0 = time.perf_counter()
        k, B, ntri = box.bispectrum(**args)                 # the first call forms the triangle counts (fp64 unit pass)
        first = time.perf_counter() - t0
        for _ in range(2):
            box.bispectrum(**args)
        eng.sync()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            box.bispectrum(**args)                          # ends in a synchronise of the stream
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(times))
        fft = phase(box, args, a.reps, ("fft_strided", "fft_contig"), 1)
        split_all, split = phase(box, args, a.reps, ("bin",), 1), phase(box, args, a.reps, ("bin",), 2)
        con_all, con = phase(box, args, a.reps, ("pca",), 1), phase(box, args, a.reps, ("pca",), 2)
        nbytes = nb * N ** 3 * (4 if prec == "f32" else 8)
        flops = 2. * 16 * 16 * nb * N ** 3
        print("N=%d %s nb=%d (%d of %d triples with triangles, ntri <= %.3g): first call %.1f ms; call median %8.3f ms (min "
              "%8.3f, max %8.3f; %d calls); split %7.3f ms; transforms %8.3f ms; contraction %8.3f ms; finishing kernels %6.3f "
              "ms; contraction: %7.1f MB read -> %5.1f%% of 8 TB/s, %.3g fp64 flops -> %5.1f%% of %.1f Tflop/s"
              % (N, prec, nb, np.count_nonzero(ntri > 0), ntri.size, ntri.max(), first * 1e3, med * 1e3, min(times) * 1e3,
                 max(times) * 1e3, a.reps, split * 1e3, fft * 1e3, con * 1e3, ((split_all - split) + (con_all - con)) * 1e3,
                 nbytes / 1e6, 100. * nbytes / con / HBM, flops, 100. * flops / con / MATRIX_FP64, MATRIX_FP64 / 1e12))
        sys.stdout.flush()
        if N in host_sizes and N not in done_host:
            done_host.add(N)
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import bk_numpy as bk
            h = np.asarray(d)
            t0 = time.perf_counter()
            ref = bk.bispectrum(h, (box.Lx, box.Ly, box.Lz), edges)
            print("    host numpy statement N=%d nb=%d (float64, BLAS threads as configured): %.2f s; ntri equal: %s"
                  % (N, nb, time.perf_counter() - t0, np.array_equal(ref["ntri"], ntri)))
            del h, ref
        del box, d
        sys.stdout.flush()


if __name__ == "__main__":
    main()
