"""Measurement aid (GPU): in-painting by constrained realisations at 128^3 and 512^3 -- median HIP-event time and TFLOP/s of one
fb_los_matmul (2 N^4 flops; fp64 operand), the time of one preconditioned CG iteration (three such products and the two per-row
kernels: the whole call minus the call stopped after one iteration, per further iteration), the whole gaussian_cr_1d call on a
cube with 5 % of the channels flagged everywhere and 1 % of the voxels at random, and from the same run fb_rotated_covariance,
whose product X V has the same flop count as one fb_los_matmul.

    python tools/inpaint_bench.py [--sizes 128,512] [--prec f32] [--reps 5]"""
import argparse
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--prec", default="f32")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print("in-painting, %s plan; median ms of %d calls" % (a.prec, a.reps))
    for N in [int(x) for x in a.sizes.split(",")]:
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision=a.prec, rng="device", seed=1,
                       stream=stream or None)
        eng = box.engine
        rs = np.random.RandomState(1)
        S = inpaint.simple_signal_cov(np.arange(N, dtype=np.float64), 1.0, N / 12.)
        var = np.full(N, 1e-2)
        rS = inpaint._sqrt_psd(S)
        d = eng.empty("real")
        w = eng.empty("real")
        wc = np.ones(N)
        wc[rs.choice(N, size=max(1, N // 20), replace=False)] = 0.
        for ix in range(N):                                             # plane by plane: no N^3 host array in fp64
            dp = rs.standard_normal((N, N)) @ rS.T + 0.1 * rs.standard_normal((N, N))
            wp = np.where(rs.uniform(size=(N, N)) < 0.01, 0., 1.) * wc
            for dev, h in ((d, dp), (w, wp)):
                h = np.ascontiguousarray(h, dtype=eng.rdtype)
                _lib.call("fb_memcpy_h2d", dev.ptr + ix * h.nbytes, h.ctypes.data, h.nbytes, eng.stream)
        # one product
        n3 = N ** 3 * 8
        X, Y, M = eng._alloc_bytes(n3), eng._alloc_bytes(n3), eng.upload_raw(rS)
        _lib.call("fb_los_matmul", eng._plan, M.ptr, d.ptr, 0, None, None, None, X.ptr, eng.stream)
        flops = 2. * N ** 4
        _, t_mm = timed(lambda: _lib.call("fb_los_matmul", eng._plan, M.ptr, X.ptr, 1, None, None, None, Y.ptr, eng.stream), a.reps)
        _, t_mm_ep = timed(lambda: _lib.call("fb_los_matmul", eng._plan, M.ptr, X.ptr, 1, None, X.ptr, X.ptr, Y.ptr, eng.stream), a.reps)
        _, t_mm_pl = timed(lambda: _lib.call("fb_los_matmul", eng._plan, M.ptr, d.ptr, 0, None, None, None, Y.ptr, eng.stream), a.reps)
        del X, Y
        # the same product inside fb_rotated_covariance
        vt = eng.upload_raw(np.ascontiguousarray(np.linalg.qr(rs.normal(size=(N, N)))[0]))
        work, cov = eng._alloc_bytes((N ** 3 + N) * 8), eng._alloc_bytes(N * N * 8)
        _, t_rot = timed(lambda: _lib.call("fb_rotated_covariance", eng._plan, d.ptr, vt.ptr, work.ptr, cov.ptr, eng.stream), a.reps)
        del work, cov
        # the whole call
        res = {}

        def call(maxiter=10000):
            out, info = inpaint.gaussian_cr_1d(d, w, S, var, realisations=1, add_noise=True, cg_maxiter=maxiter, verbose=False,
                                               box=box, return_info=True)
            res[maxiter] = info
            return out
        _, t_call = timed(call, a.reps)
        info = res[10000]
        n_it = int(info.n_iter_host().max())
        _, t_one = timed(lambda: call(1), a.reps)
        _, t_wiener = timed(lambda: inpaint.wiener_filter_1d(d, w, S, var, box=box), a.reps)
        print("N = %d   (%d of %d channels flagged everywhere + 1 %% of the voxels)" % (N, int((wc == 0).sum()), N))
        print("  fb_los_matmul         %8.3f ms   %6.2f TFLOP/s   fp64 operand, no epilogue; model: X read, Y written, %d MB -> %.3f ms at 5 TB/s"
              % (t_mm, flops / t_mm * 1e-9, 2 * n3 // 2 ** 20, 2 * n3 / 5e12 * 1e3))
        print("    with post and add   %8.3f ms   %6.2f TFLOP/s" % (t_mm_ep, flops / t_mm_ep * 1e-9))
        print("    plan-precision X    %8.3f ms   %6.2f TFLOP/s" % (t_mm_pl, flops / t_mm_pl * 1e-9))
        print("  fb_rotated_covariance %8.3f ms   the same flop count in its product X V (wave reductions), then the covariance" % t_rot)
        print("  gaussian_cr_1d        %8.3f ms   one realisation with added noise: %d CG iterations at most, residual %.2e, %d of %d "
              "converged; host: eigh of S and of P^-1" % (t_call, n_it, info.residual, info.converged, N * N))
        print("  per CG iteration      %8.3f ms   (the whole call - the call stopped after 1 iteration) / %d: 3 products, 2 per-row kernels, "
              "one read-back" % ((t_call - t_one) / max(1, n_it - 1), n_it - 1))
        print("  wiener_filter_1d      %8.3f ms" % t_wiener)
        del box, eng, d, w
    return 0


if __name__ == "__main__":
    sys.exit(main())
