"""Measurement aid (GPU): the LSSA delay spectrum of a flagged cube at 128^3 and 512^3, Ntau = N -- median HIP-event time of the
fused call (fb_lssa through inpaint.lssa_delay_spectrum's prepared inputs: the row sums, the fused kernel, the two reduction
kernels and the read-back of the averages) with per-channel and with per-voxel flags, without and with the three per-row
outputs stored, and the TFLOP/s of its model (4 N^3 Ntau flops with per-channel flags, 8 N^3 Ntau with per-voxel ones); and the
same averages composed from what the library offered before: fb_gcr_rhs (u = q d), one fb_los_matmul per product (two, or four
with per-voxel flags), the downloads, and the division, rotation, power and average in numpy on the host (wall clock, once).

    python tools/lssa_bench.py [--sizes 128,512] [--prec f32] [--reps 5]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, inpaint, _lib                 # noqa: E402


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


def composed(eng, d, w_dev, w_kind, wc, var_dev, cos, sin):
    """(ps_mean, seconds): the parent's route.  Row by row it is the statement of tests/lssa_numpy.py."""
    N = eng.N
    n3 = N ** 3 * 8
    t0 = time.perf_counter()
    q, u = eng._alloc_bytes(n3), eng._alloc_bytes(n3)
    _lib.call("fb_gcr_rhs", eng._plan, d.ptr, w_dev.ptr, w_kind, var_dev.ptr, 0, None, 0, 0, 0, q.ptr, u.ptr, None, None, eng.stream)

    def product(M, X_ptr, kind):
        Y, h = eng._alloc_bytes(n3), np.empty((N * N, N))
        _lib.call("fb_los_matmul", eng._plan, eng.upload_raw(np.ascontiguousarray(M)).ptr, X_ptr, kind, None, None, None, Y.ptr, eng.stream)
        _lib.call("fb_memcpy_d2h", h.ctypes.data_as(ctypes.c_void_p), Y.ptr, h.nbytes, eng.stream)
        return h
    uc, us = product(cos, u.ptr, 1), product(sin, u.ptr, 1)
    G = product(np.ones((N, N)), q.ptr, 1)[:, 0].copy()               # the row sums of q, by the same product
    if w_kind == 1:                                                     # flags are 0 / 1: w^2 = w
        Scc, Scs = product(cos * cos, w_dev.ptr, 0), product(cos * sin, w_dev.ptr, 0)
        Sss = product(np.ones((N, N)), w_dev.ptr, 0)[:, :1] - Scc
    else:
        c, s = wc * cos, wc * sin
        Scc, Scs, Sss = [np.sum(x, axis=1)[None, :] for x in (c * c, c * s, s * s)]
    on = G > 0.
    with np.errstate(all="ignore"):
        A_re, A_im = uc / G[:, None], -us / G[:, None]
        th = 0.5 * np.arctan2(2. * Scs, Scc - Sss)
        c, s = np.cos(th), np.sin(th)
        l0 = c * c * Scc + 2. * s * c * Scs + s * s * Sss
        l1 = s * s * Scc - 2. * s * c * Scs + c * c * Sss
        ps = (((c * A_re + s * A_im) * l1) ** 2 + ((-s * A_re + c * A_im) * l0) ** 2) / (l0 ** 2 + l1 ** 2)
    mean = ps[on].mean(axis=0)
    return mean, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print("LSSA delay spectrum, %s plan, Ntau = N; fused: median ms of %d calls; composed: wall clock of one call" % (a.prec, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=a.prec, rng="device", seed=1,
                       stream=stream or None)
        eng = box.engine
        rs = np.random.RandomState(1)
        d, w = eng.empty("real"), eng.empty("real")
        wc = np.ones(N)
        wc[rs.choice(N, size=max(1, N // 10), replace=False)] = 0.
        for ix in range(N):                                             # plane by plane: no N^3 host array in fp64
            dp = rs.standard_normal((N, N))
            wp = np.where(rs.uniform(size=(N, N)) < 0.01, 0., 1.) * wc
            for dev, h in ((d, dp), (w, wp)):
                h = np.ascontiguousarray(h, dtype=eng.rdtype)
                _lib.call("fb_memcpy_h2d", dev.ptr + ix * h.nbytes, h.ctypes.data, h.nbytes, eng.stream)
        freqs = 1000. + 0.5 * np.arange(N, dtype=np.float64)[::-1]
        var = rs.uniform(0.5, 2.0, size=N)
        print("N = %d   (%d of %d channels flagged everywhere; per-voxel flags: + 1 %% of the voxels)" % (N, int((wc == 0).sum()), N))
        for name, flags, nprod in (("per-channel flags", wc, 2), ("per-voxel flags", w, 4)):
            inp = inpaint._LSSAInputs(d, flags, freqs, var, None, None, box)
            flops = 2. * nprod * N ** 3 * inp.tau.size
            (mean, err, n_los), t = timed(lambda: inp.run(True, None, None, None), a.reps)
            bufs = [inp.rows() for _ in range(3)]
            _, t_keep = timed(lambda: inp.run(True, *bufs), a.reps)
            del bufs
            phi = inpaint.lssa_phase(inp.tau, freqs)
            ref, t_comp = composed(eng, d, inp.w, inp.w_kind, wc, inp.var, np.cos(phi), np.sin(phi))
            dev = float(np.max(np.abs(mean - ref)) / np.max(np.abs(ref)))
            print("  %-18s fused %9.3f ms  %6.2f TFLOP/s (model %d N^3 Ntau flops)   with A_re, A_im, ps stored %9.3f ms   "
                  "composed %9.1f ms (%d fb_los_matmul + downloads + numpy)   ps_mean fused against composed %.1e, n_los %d"
                  % (name, t, flops / t * 1e-9, 2 * nprod, t_keep, t_comp * 1e3, nprod + (2 if nprod == 4 else 1), dev, n_los))
        del box, eng, d, w
    return 0


if __name__ == "__main__":
    sys.exit(main())
