"""Measurement aid (GPU): NMF, ICA and band-power PCA cleaning at 128^3 and 512^3 -- median HIP-event time of one NMF iteration
(fb_nmf_sweep: one pass over the cube), of one FastICA step (fb_ica_step) and of the whole calls, each bracketed by events on
the box's stream, warm-up excluded, with a byte model for comparison; and the numpy statement (tests/cleaning_numpy.py) of the
NMF and ICA calls at 64^3 on the host, for scale.

    python tools/cleaning_bench.py [--sizes 128,512] [--prec f32] [--nmodes 3] [--reps 5] [--host-size 64]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, filters, _lib                 # noqa: E402
from tests import cleaning_numpy as cn                                         # noqa: E402


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


def device_cube(eng, N, seed=1):
    """The test cubes' recipe (three positive maps times power laws plus small positive noise), built plane by plane."""
    rng = np.random.RandomState(seed)
    nu = np.linspace(1., 2., N)
    maps = [rng.uniform(0.5, 1.5, size=(N, N)), np.abs(rng.laplace(0., 0.3, size=(N, N)) + 1.) + 0.05,
            np.abs(np.sin(3. * rng.normal(size=(N, N)))) + 0.05]
    host = np.empty((N, N, N), dtype=eng.rdtype)
    for ix in range(N):
        plane = 1e-2 * rng.uniform(0.05, 1., size=(N, N))
        for m, (beta, amp) in zip(maps, cn.SPECTRA):
            plane += m[ix][:, None] * (amp * nu ** beta)[None, :]
        host[ix] = plane
    return eng.upload(host, "real")


def host(N, k):
    X = cn.as_matrix(cn.build_cube(N))
    t0 = time.time()
    r = cn.nmf(X, k)
    t1 = time.time()
    q = cn.fastica(X, k, random_state=0)
    t2 = time.time()
    print("numpy statement, N = %d, nmodes = %d, host: NMF %.0f ms (%d iterations), ICA %.0f ms (%d iterations)"
          % (N, k, (t1 - t0) * 1e3, r["n_iter"], (t2 - t1) * 1e3, q["n_iter_"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--nmodes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-size", type=int, default=64)
    a = ap.parse_args()
    k = a.nmodes
    print("foreground cleaning, %s plan, nmodes = %d; median ms of %d calls" % (a.prec, k, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=a.prec, stream=stream or None)
        eng = box.engine
        cube = device_cube(eng, N)
        npix, b = N * N, 4 if a.prec == "f32" else 8
        (W, H), t_init = timed(lambda: filters._nndsvda(eng, cube, k), a.reps)
        vt = eng.upload_raw(np.ascontiguousarray(np.linalg.qr(np.random.RandomState(2).normal(size=(N, N)))[0]))
        work, cov = eng._alloc_bytes((N ** 3 + N) * 8), eng._alloc_bytes(N * N * 8)
        _, t_rot = timed(lambda: _lib.call("fb_rotated_covariance", eng._plan, cube.ptr, vt.ptr, work.ptr, cov.ptr, eng.stream), a.reps)
        del work, cov
        v = np.empty(2)
        _, t_it = timed(lambda: _lib.call("fb_nmf_sweep", eng._plan, cube.ptr, W.ptr, H.ptr, k, v.ctypes.data_as(_lib.P_double),
                                          eng.stream), a.reps)
        (_, res), t_nmf = timed(lambda: filters.nmf_filter(cube, k, return_filter=True), a.reps)
        it_bytes = b * N ** 3 + 2 * 8 * k * npix
        print("N = %d" % N)
        print("  NMF iteration %8.3f ms   model: the cube once (%d B per value) + W read and written, %.0f MB -> %.3f ms at 5 TB/s"
              " (+ the partials' finish, the H half in one workgroup and one read-back)" % (t_it, b, it_bytes / 1e6, it_bytes / 5e12 * 1e3))
        print("  NNDSVDA       %8.3f ms   means, covariance, eigh on the host, the rotated pass (X V in fp64 and its covariance),"
              " eigh and SVD of N x N on the host, projection" % t_init)
        print("  of which fb_rotated_covariance %8.3f ms   model: the cube once + X V written and read in fp64, %.0f MB -> %.3f ms"
              " at 5 TB/s; N^3 wave reductions and V (N^2 doubles) from cache per pixel" % (t_rot, (b + 16) * N ** 3 / 1e6,
                                                                                         (b + 16) * N ** 3 / 5e12 * 1e3))
        print("  nmf_filter    %8.3f ms   %d iterations + NNDSVDA + residual" % (t_nmf, res.n_iter_))
        (_, ica), t_ica = timed(lambda: filters.ica_filter(cube, k, return_filter=True, random_state=0), a.reps)
        X1 = eng._alloc_bytes(k * npix * 8)
        _lib.call("fb_memcpy_d2d", X1.ptr, ica.sources.ptr, k * npix * 8, eng.stream)
        Wm, G, gp = np.eye(k), np.empty((k, k)), np.empty(k)
        _, t_st = timed(lambda: _lib.call("fb_ica_step", eng._plan, Wm.ctypes.data_as(_lib.P_double), X1.ptr, k, 0, 1.0,
                                          G.ctypes.data_as(_lib.P_double), gp.ctypes.data_as(_lib.P_double), eng.stream), a.reps)
        _, t_pca = timed(lambda: filters.pca_filter(cube, k), a.reps)
        print("  ICA step      %8.3f ms   model: X1 once, %.0f MB -> %.3f ms at 5 TB/s (+ upload of W, read-back of G; timed on the unit-variance sources in place of X1)"
              % (t_st, 8 * k * npix / 1e6, 8 * k * npix / 5e12 * 1e3))
        print("  ica_filter    %8.3f ms   with the filter: %d iterations, whitening, sources; cleaned cube only = pca_filter: %.3f ms"
              % (t_ica, ica.n_iter_, t_pca))
        _, t_bp = timed(lambda: filters.bandpower_pca_filter(cube, 3, k), a.reps)
        print("  bandpower_pca %8.3f ms   3 bands: band-pass (two transverse transforms of a complex cube) + PCA each" % t_bp)
        del box
    host(a.host_size, k)


if __name__ == "__main__":
    main()
