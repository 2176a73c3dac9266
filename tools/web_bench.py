"""Measurement aid (GPU): the three cosmic-web kernels -- fb_tidal_k, fb_shear_k and fb_web_eigen (one threshold with the
eigenvalue and class cubes written; sixteen thresholds with a weight, counts and sums only) -- at 256^3 and 512^3 in f32 and
f64, timed with HIP events on the box's stream (median of --reps calls after one warm-up; all buffers already on the device,
filled with a Gaussian realisation and its tidal tensor).  Beside each time, the yardstick: a plain device-to-device copy that
moves the same number of bytes (half of them read, half written), timed the same way.  ``bytes`` counts the elements a kernel
has to touch: the stored modes N x N x (N/2 + 1) of every spectrum read or written, the N^3 voxels of every cube.
``ratio`` = kernel time / copy time; ``fp64_gflops`` for the eigen pass uses the operation count of DESIGN.md section 4.

    python tools/web_bench.py [--precs f32,f64] [--sizes 256,512] [--reps 5]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, _lib, web                    # noqa: E402
from fastbox_amd.device import HALF, REAL                                      # noqa: E402

EIGEN_FLOPS = 18 * 22 + 20                      # per voxel: 6 sweeps x 3 rotations of 22 operations, sort, class


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


def copy_ms(eng, nbytes, reps):
    half = (nbytes // 2 + 255) & ~255
    src, dst = eng._alloc_bytes(half), eng._alloc_bytes(half)
    return median_ms(lambda: _lib.call("fb_memcpy_d2d", dst.ptr, src.ptr, half, eng.stream), reps)


def rows(box, reps):
    eng, N = box.engine, box.N
    item = np.dtype(eng.rdtype).itemsize
    spec, cube = N * N * (N // 2 + 1) * 2 * item, N ** 3 * item
    delta = box.realise_density(inplace=False)
    dk = eng.fft_r2c(delta)
    out = [eng.empty(HALF) for _ in range(6)]
    vk = [eng.velocity_k(dk, c, 50.) for c in range(3)]

    def row(kernel, ms, nbytes, **kw):
        cp = copy_ms(eng, nbytes, reps)
        r = dict(what=kernel, prec=eng.precision, N=N, ms=round(ms, 3), bytes=nbytes, copy_ms=round(cp, 3), ratio=round(ms / cp, 2),
                 gbyte_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1))
        r.update(kw)
        return r
    ms = median_ms(lambda: _lib.call("fb_tidal_k", eng._plan, dk.ptr, web._ptrs(out), 4., eng.stream), reps)
    yield row("fb_tidal_k", ms, 7 * spec)
    ms = median_ms(lambda: _lib.call("fb_shear_k", eng._plan, web._ptrs(vk), web._ptrs(out), 4., 70., eng.stream), reps)
    yield row("fb_shear_k", ms, 9 * spec)
    del out, vk
    T = web.tidal_tensor(box, delta_k=dk, smoothing=4.)
    del dk
    eig = [eng.empty(REAL) for _ in range(3)]
    classes = eng._alloc_bytes(N ** 3)
    comps = web._ptrs(T.components)
    one = np.zeros(1)
    ms = median_ms(lambda: _lib.call("fb_web_eigen", eng._plan, comps, one.ctypes.data_as(_lib.P_double), 1, 0, None,
                                     web._ptrs(eig), classes.ptr, None, None, None, eng.stream), reps)
    yield row("fb_web_eigen nt=1, eigenvalues and classes", ms, 9 * cube + N ** 3,
              fp64_gflops=round(EIGEN_FLOPS * float(N) ** 3 / (ms * 1e-3) / 1e9, 1))
    del eig, classes
    thr = np.linspace(-0.05, 0.1, 16)
    counts, wsum, n_nan = np.zeros(64, dtype=np.uint64), np.zeros(64), ctypes.c_uint64(0)
    P_u64 = ctypes.POINTER(ctypes.c_uint64)
    ms = median_ms(lambda: _lib.call("fb_web_eigen", eng._plan, comps, thr.ctypes.data_as(_lib.P_double), 16, 0, delta.ptr, None,
                                     None, counts.ctypes.data_as(P_u64), wsum.ctypes.data_as(_lib.P_double), ctypes.byref(n_nan),
                                     eng.stream), reps)
    yield row("fb_web_eigen nt=16, counts and weight sums", ms, 7 * cube,
              fp64_gflops=round((EIGEN_FLOPS + 16 * 11) * float(N) ** 3 / (ms * 1e-3) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for prec in [x for x in a.precs.split(",") if x]:
        for N in [int(x) for x in a.sizes.split(",") if x]:
            box = make_box(N, prec)
            for r in rows(box, a.reps):
                print(json.dumps(r), flush=True)
            box.engine.release_idle_buffers()
            del box
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
