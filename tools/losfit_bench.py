"""Measurement aid (GPU): the line-of-sight foreground fits at 512^3 on both plans, with and without a weight cube -- median
HIP-event time of the two fit kernels (fb_los_polyfit at order 3 in ln T against ln nu, fb_los_powerlaw; tables uploaded
beforehand, the one read-back of the failure count included), gpr_filter split into Gram matrix, host optimisation and
projection (host clock around synchronised stages, GPRResult.timings), and pca_filter(nmodes=4) in the same run as the
yardstick; each kernel beside its model bytes over 8 TB/s.

    python tools/losfit_bench.py [--sizes 512] [--precs f32,f64] [--reps 5] [--restarts 10]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, filters, losfit, _lib         # noqa: E402

PEAK = 8e12        # bytes per second: the HBM3E figure of the data sheet


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


def device_cubes(eng, N, freqs, seed=1):
    """A power law per pixel (amplitude 5 .. 20, index -2.9 .. -2.5) plus a free-free term and 1e-5 relative noise, and a weight
    cube with 20 % of the voxels flagged; built plane by plane."""
    rng = np.random.RandomState(seed)
    lnx = np.log(freqs / freqs[0])
    data, w = np.empty((N, N, N), dtype=eng.rdtype), np.empty((N, N, N), dtype=eng.rdtype)
    for ix in range(N):
        amp, beta = rng.uniform(5., 20., size=(N, 1)), rng.uniform(-2.9, -2.5, size=(N, 1))
        plane = amp * np.exp(beta * lnx) + 0.05 * amp * np.exp(-2.1 * lnx)
        data[ix] = plane * (1. + 1e-5 * rng.standard_normal((N, N)))
        w[ix] = np.where(rng.uniform(size=(N, N)) < 0.2, 0., rng.uniform(0.5, 1.5, size=(N, N)))
    return eng.upload(data, "real"), eng.upload(w, "real")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restarts", type=int, default=10)
    a = ap.parse_args()
    print("line-of-sight foreground fits; median ms of %d calls; model = bytes over 8 TB/s" % a.reps)
    for N in [int(x) for x in a.sizes.split(",")]:
        for prec in a.precs.split(","):
            stream = torch.cuda.current_stream().cuda_stream
            box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=prec, stream=stream or None)
            eng = box.engine
            npix, b = N * N, 4 if prec == "f32" else 8
            freqs = np.linspace(900., 1050., N)
            cube, wcube = device_cubes(eng, N, freqs)
            order = 3
            basis = losfit.legendre_basis(np.log(freqs), order)
            pinv = eng.upload_raw(np.ascontiguousarray(np.linalg.pinv(basis.T)))
            basis_dev = eng.upload_raw(basis)
            lnx = eng.upload_raw(np.ascontiguousarray(np.log(freqs / freqs[0])))
            out = eng.empty("real")
            status, n_iter, rows = eng._alloc_bytes(npix * 4), eng._alloc_bytes(npix * 4), eng._alloc_bytes(5 * npix * 8)
            nf = ctypes.c_int32(0)
            print("N = %d, %s plan" % (N, prec))
            for label, wbuf, pbuf in (("no weights (shared pseudo-inverse)", None, pinv), ("weight cube (Cholesky per row)", wcube, None)):
                nbytes = b * N ** 3 * (2 + (wbuf is not None))
                _, t = timed(lambda: _lib.call("fb_los_polyfit", eng._plan, cube.ptr, wbuf.ptr if wbuf is not None else None, 1, basis_dev.ptr,
                                               pbuf.ptr if pbuf is not None else None, order, 1, out.ptr, None, None, None, status.ptr,
                                               ctypes.byref(nf), eng.stream), a.reps)
                print("  fb_los_polyfit   %8.3f ms   %-36s model: %4.0f MB -> %.3f ms; %d rows failed" % (t, label, nbytes / 1e6, nbytes / PEAK * 1e3, nf.value))
                _, t = timed(lambda: _lib.call("fb_los_powerlaw", eng._plan, cube.ptr, None, None, 0, wbuf.ptr if wbuf is not None else None, 1, lnx.ptr,
                                               -2.1, None, 50, 1e-12, out.ptr, None, rows.ptr, n_iter.ptr, status.ptr, ctypes.byref(nf),
                                               eng.stream), a.reps)
                it = np.empty(npix, dtype=np.int32)
                _lib.call("fb_memcpy_d2h", it.ctypes.data_as(ctypes.c_void_p), n_iter.ptr, it.nbytes, eng.stream)
                print("  fb_los_powerlaw  %8.3f ms   %-36s model: %4.0f MB -> %.3f ms; %d rows failed, %.1f steps per row" % (
                    t, "weight cube" if wbuf is not None else "no weights", nbytes / 1e6, nbytes / PEAK * 1e3, nf.value, it.mean()))
            tg = []
            for _ in range(max(1, a.reps // 2)):
                _, res = filters.gpr_filter(cube, return_filter=True, opt_messages=False, opt_num_restarts=a.restarts)
                tg.append([res.timings[k] * 1e3 for k in ("gram", "optimise", "project")])
            tg = np.median(np.array(tg), axis=0)
            print("  gpr_filter       %8.3f ms   Gram %.3f ms (model: the cube twice, %.0f MB -> %.3f ms), host optimisation %.3f ms (%d starts), "
                  "projection %.3f ms (model: the cube once, an fp64 cube written and read, the result, %.0f MB -> %.3f ms)" % (
                      tg.sum(), tg[0], 2 * b * N ** 3 / 1e6, 2 * b * N ** 3 / PEAK * 1e3, tg[1], res.n_starts, tg[2],
                      (2 * b + 16) * N ** 3 / 1e6, (2 * b + 16) * N ** 3 / PEAK * 1e3))
            _, t = timed(lambda: filters.pca_filter(cube, nmodes=4), a.reps)
            print("  pca_filter(4)    %8.3f ms   the yardstick (model: the cube three times and the result, %.0f MB -> %.3f ms)" % (
                t, 4 * b * N ** 3 / 1e6, 4 * b * N ** 3 / PEAK * 1e3))
            del cube, wcube, out, box


if __name__ == "__main__":
    main()
