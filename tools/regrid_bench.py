"""Measurement aid (GPU): fb_regrid_trilinear for 256 x 256 x 512 -> 512^3 and 512^3 -> 512^3 in f32 and f64, and
fb_grid_catalogue for the 256^3 particles of a COLA run onto 256^3 beside fb_paint with the NGP window on the same particles,
timed with HIP events on the box's stream (median of --reps calls after one warm-up; cube, tables and particles already on the
device).  The regrid call is the locate kernel, the channel-mean pass and the interpolation kernel; its byte model is the input
read once plus the output written once, over 8 TB/s -- the mean pass reads the input a second time, which the second model
counts.  Both indexings are timed: 'ij' reads adjacent input rows, 'xy' rows of different x planes.  And the host reference
at each of --host-sizes: scipy's RegularGridInterpolator behind the NaN fill for
(s/2) x (s/2) x s -> s^3, and np.histogramdd for s^3 particles onto s^3, one core.

    python tools/regrid_bench.py [--precs f32,f64] [--reps 5] [--size 512] [--cola-size 256] [--host-sizes 128,256] [--no-cola]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, _lib                         # noqa: E402

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


def regrid(box, shape, reps, swap):
    eng, N = box.engine, box.N
    item = np.dtype(eng.rdtype).itemsize
    if shape == (N, N, N):
        cube = box.realise_density(inplace=False)
    else:
        cube = eng.upload_raw(np.random.RandomState(1).standard_normal(shape).astype(eng.rdtype))
    g = [np.arange(n, dtype=np.float64) for n in shape]
    p = [0.25 + (n - 1.5) * np.arange(N) / (N - 1.) for n in shape]          # inside the nodes, off them
    tabs = eng.upload_raw(np.concatenate(g + p))
    ptr, off = [], 0
    for q in g + p:
        ptr.append(tabs.ptr + 8 * off)
        off += q.size
    out = eng.empty("real")

    def call():
        _lib.call("fb_regrid_trilinear", eng._plan, cube.ptr, shape[0], shape[1], shape[2], ptr[0], ptr[1], ptr[2],
                  ptr[3], N, ptr[4], N, ptr[5], N, swap, out.ptr, eng.stream)
    ms = median_ms(call, reps)
    nin, nout = float(np.prod(shape)) * item, float(N) ** 3 * item
    return dict(what="regrid", prec=eng.precision, indexing="xy" if swap else "ij", shape="%dx%dx%d -> %d^3" % (shape + (N,)), ms=round(ms, 3),
                model_ms=round(1e3 * (nin + nout) / PEAK, 3), model_two_reads_ms=round(1e3 * (2 * nin + nout) / PEAK, 3),
                tb_per_s=round((nin + nout) / (ms * 1e-3) / 1e12, 3))


def catalogue(N, prec, reps):
    box = make_box(N, prec)
    eng = box.engine
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, seed=12, return_particles=True, inplace=False)
    eng.release_idle_buffers()
    n = parts.n
    edges = np.linspace(0., float(box.Lx), N + 1)
    etab = eng.upload_raw(edges)
    out = eng.empty("real")
    t_grid = median_ms(lambda: _lib.call("fb_grid_catalogue", eng._plan, parts.ptr, None, n, etab.ptr, N, etab.ptr, N, etab.ptr, N,
                                         out.ptr, eng.stream), reps)
    t_ngp = median_ms(lambda: _lib.call("fb_paint", eng._plan, parts.ptr, None, n, 0, out.ptr, eng.stream), reps)
    return dict(what="grid_catalogue", prec=prec, particles="%d^3" % N, cells="%d^3" % N, ms=round(t_grid, 3),
                fb_paint_ngp_ms=round(t_ngp, 3))


def host(s):
    from scipy.interpolate import RegularGridInterpolator
    rs = np.random.RandomState(2)
    shape = (s // 2, s // 2, s)
    f = rs.standard_normal(shape)
    g = [np.arange(n, dtype=np.float64) for n in shape]
    p = [0.25 + (n - 1.5) * np.arange(s) / (s - 1.) for n in shape]
    t0 = time.time()
    interp = RegularGridInterpolator(tuple(g), f, method="linear", bounds_error=False, fill_value=np.nan)
    x3, y3, z3 = np.meshgrid(*p)
    interp(np.array([x3.flatten(), y3.flatten(), z3.flatten()]).T).reshape(x3.shape)
    t1 = time.time()
    pos = rs.random_sample((s ** 3, 3))
    t2 = time.time()
    np.histogramdd(pos, bins=(s,) * 3, range=[(0., 1.)] * 3)
    t3 = time.time()
    return dict(what="host", regrid="%dx%dx%d -> %d^3" % (shape + (s,)), regrid_scipy_ms=round(1e3 * (t1 - t0), 1),
                particles="%d^3" % s, histogramdd_ms=round(1e3 * (t3 - t2), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--cola-size", type=int, default=256)
    ap.add_argument("--host-sizes", default="128", help="comma-separated; empty: no host reference")
    ap.add_argument("--no-cola", action="store_true")
    a = ap.parse_args()
    N = a.size
    for prec in [x for x in a.precs.split(",") if x]:
        box = make_box(N, prec)
        for shape in ((N // 2, N // 2, N), (N, N, N)):
            for swap in (1, 0):
                print(json.dumps(regrid(box, shape, a.reps, swap)), flush=True)
            box.engine.release_idle_buffers()
        del box
        torch.cuda.empty_cache()
        if not a.no_cola:
            print(json.dumps(catalogue(a.cola_size, prec, a.reps)), flush=True)
    for s in [int(x) for x in a.host_sizes.split(",") if x]:
        print(json.dumps(host(s)), flush=True)


if __name__ == "__main__":
    main()
