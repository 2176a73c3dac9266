"""Measurement aid (GPU): the three interferometer kernels and Interferometer.observe at 512^3 for a 331-element hexagonal
array with 1 and 32 hour angles.  Per piece the median over calls of the HIP-event time around the call on the box's stream.

  fb_uv_coverage (accumulate = 1: the kernel without the clearing of the cube, which is timed on its own) on four sample sets:
    the array's baselines collapsed to distinct ones with multiplicities (what Interferometer sends), a random set of the same
    size, the baselines as they come (every redundant copy its own sample), a random set of that size.  Models: the guide's
    chip-wide atomic rate for float adds, 1.3 TB/s of added bytes, applied to 2 ns N 4 bytes; a device copy of the N^3 int32 cube.
  fb_uv_channel_sums, fb_uv_weight (three modes): against a device copy of the bytes they touch.
  observe end to end (coverage cached), and the first call that computes the coverage.
  --numpy N: the numpy statement of the coverage on one host core at grid N (no GPU needed).

    python tools/interferometer_bench.py [--size 512] [--precs f32] [--reps 10] [--numpy 128]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
from fastbox_amd import interferometer as itf                                  # noqa: E402

LAT = np.radians(-30.7)
ATOMIC_RATE = 1.3e12            # bytes / s of added bytes, float adds (the kernel guide)


def array_samples(sx, sy, N, nt):
    """(samples as they come, nt hour angles) of the 331-element hexagon scaled so that its longest baseline reaches 95 % of the
    uv grid's edge in the top channel."""
    spacing = 0.95 * (0.5 * N / max(sx.max(), sy.max())) / 20.
    bl = itf.baselines_from_antennas(itf.hex_array(11, spacing))
    if nt == 1:
        return np.ascontiguousarray(bl)
    return itf.rotation_synthesis(bl, LAT, LAT, np.linspace(-np.pi / 12., np.pi / 12., nt))


def random_samples(sx, sy, N, ns, seed):
    rs = np.random.RandomState(seed)
    r = 0.95 * 0.5 * N / max(sx.max(), sy.max())
    return np.stack([rs.uniform(-r, r, ns), rs.uniform(-r, r, ns)], axis=1)


def numpy_statement(N, nt):
    from tests import interferometer_cases as ic
    from tests import interferometer_numpy as inp
    hb = ic.HostBox(N, 1e3)
    sx, sy = itf.channel_scales(hb)
    uniq, mult = itf.collapse_samples(array_samples(sx, sy, N, nt))
    t0 = time.time()
    S = inp.coverage(N, uniq, mult, sx, sy)
    t1 = time.time()
    inp.channel_sums(S)
    t2 = time.time()
    print("numpy statement, one host core, N=%d, %d hour angle(s), %d distinct samples: coverage %.2f s (%.1f ns per sample and "
          "channel), sums %.3f s" % (N, nt, len(uniq), t1 - t0, 1e9 * (t1 - t0) / max(len(uniq) * N, 1), t2 - t1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precs", default="f32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy", type=int, default=0)
    a = ap.parse_args()
    if a.numpy:
        for nt in (1, 32):
            numpy_statement(a.numpy, nt)
        return
    import torch
    from fastbox_amd import CosmoBox, Interferometer, default_cosmo, _lib

    def timed(eng, fn, reps):
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
        return float(np.median(times))

    N = a.size
    for prec in a.precs.split(","):
        stream = torch.cuda.current_stream().cuda_stream
        box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, redshift=0.8, realise_now=False, precision=prec, rng="device",
                       seed=3, stream=stream or None)
        eng = box.engine
        tag = "N=%d %s" % (N, prec)
        sx, sy = itf.channel_scales(box)
        sx_dev, sy_dev = eng.upload_raw(sx), eng.upload_raw(sy)
        counts = eng._alloc_bytes(4 * N ** 3)
        spare = eng._alloc_bytes(4 * N ** 3)
        cube_bytes = 4 * N ** 3
        t_copy = timed(eng, lambda: _lib.call("fb_memcpy_d2d", spare.ptr, counts.ptr, cube_bytes, eng.stream), a.reps)
        print("%s device copy of the int32 cube (%.0f MB read + written): %7.3f ms -> %.2f TB/s"
              % (tag, cube_bytes / 1e6, t_copy * 1e3, 2 * cube_bytes / t_copy / 1e12))
        empty = eng.upload_raw(np.zeros(2))
        t_clear = timed(eng, lambda: _lib.call("fb_uv_coverage", eng._plan, empty.ptr, None, 0, sx_dev.ptr, sy_dev.ptr, counts.ptr, 0,
                                               eng.stream), a.reps)
        print("%s fb_uv_coverage, ns = 0 (clears the cube): %7.3f ms" % (tag, t_clear * 1e3))
        for nt in (1, 32):
            raw = array_samples(sx, sy, N, nt)
            uniq, mult = itf.collapse_samples(raw)
            sets = (("collapsed array", uniq, mult), ("random, same ns", random_samples(sx, sy, N, len(uniq), 1), mult),
                    ("array as it comes", raw, None), ("random, same ns", random_samples(sx, sy, N, len(raw), 2), None))
            t_sets = []
            for name, s, m in sets:
                s_dev = eng.upload_raw(np.ascontiguousarray(s))
                m_dev = eng.upload_raw(np.ascontiguousarray(m)) if m is not None else None
                _lib.call("fb_uv_coverage", eng._plan, None, None, 0, sx_dev.ptr, sy_dev.ptr, counts.ptr, 0, eng.stream)
                t = timed(eng, lambda: _lib.call("fb_uv_coverage", eng._plan, s_dev.ptr, m_dev.ptr if m_dev else None, len(s), sx_dev.ptr,
                                                 sy_dev.ptr, counts.ptr, 1, eng.stream), a.reps)
                added = 2. * len(s) * N * 4
                t_sets.append(t)
                print("%s coverage, %2d hour angle(s), %-17s ns = %8d: %8.3f ms; %8.1f MB added -> %6.3f TB/s (%5.1f%% of the float-add "
                      "rate); %6.2f x the cube copy" % (tag, nt, name, len(s), t * 1e3, added / 1e6, added / t / 1e12,
                                                        100. * added / t / ATOMIC_RATE, t / t_copy))
            print("%s coverage, %2d hour angle(s): collapsed array / random of equal ns = %.2f; as it comes / random of equal ns = %.2f"
                  % (tag, nt, t_sets[0] / t_sets[1], t_sets[2] / t_sets[3]))
        # the cube the other two kernels see: the collapsed array's, 32 hour angles
        uniq, mult = itf.collapse_samples(array_samples(sx, sy, N, 32))
        s_dev, m_dev = eng.upload_raw(uniq), eng.upload_raw(mult)
        _lib.call("fb_uv_coverage", eng._plan, s_dev.ptr, m_dev.ptr, len(uniq), sx_dev.ptr, sy_dev.ptr, counts.ptr, 0, eng.stream)
        sums = eng._alloc_bytes(16 * N)
        t = timed(eng, lambda: _lib.call("fb_uv_channel_sums", eng._plan, counts.ptr, sums.ptr, eng.stream), a.reps)
        print("%s fb_uv_channel_sums: %7.3f ms; %.0f MB read -> %.2f TB/s; %.2f x a device copy of as many bytes (read + written)"
              % (tag, t * 1e3, cube_bytes / 1e6, cube_bytes / t / 1e12, t / (t_copy / 2)))
        full = eng.empty("full")
        _lib.call("fb_uv_coverage", eng._plan, None, None, 0, sx_dev.ptr, sy_dev.ptr, full.ptr, 0, eng.stream)      # zeros: finite values
        full_bytes = eng.nbytes["full"]
        t_fcopy = timed(eng, lambda: _lib.call("fb_memcpy_d2d", spare.ptr, full.ptr, cube_bytes, eng.stream), a.reps) * (
            (2. * full_bytes + cube_bytes) / (2. * cube_bytes))
        scale_dev = eng.upload_raw(np.ones(N))
        for mode, name in ((0, "natural"), (1, "uniform"), (2, "sqrt")):
            t = timed(eng, lambda: _lib.call("fb_uv_weight", eng._plan, full.ptr, counts.ptr, mode, scale_dev.ptr, eng.stream), a.reps)
            moved = 2 * full_bytes + cube_bytes
            print("%s fb_uv_weight %-7s: %7.3f ms; %.0f MB moved -> %.2f TB/s; %.2f x a device copy moving as many bytes"
                  % (tag, name, t * 1e3, moved / 1e6, moved / t / 1e12, t / t_fcopy))
        del full, counts, spare
        # end to end
        for nt in (1, 32):
            spacing = 0.95 * (0.5 * N / max(sx.max(), sy.max())) / 20.
            kw = {} if nt == 1 else dict(latitude=LAT, declination=LAT, hour_angles=np.linspace(-np.pi / 12., np.pi / 12., nt))
            sky = eng.empty("real")
            one = np.ones(N)
            _lib.call("fb_sky_noise_cube", eng._plan, one.ctypes.data_as(_lib.P_double), None, 5, sky.ptr, eng.stream)
            eng.sync()
            t0 = time.time()
            inst = Interferometer(box, antennas=itf.hex_array(11, spacing), **kw)
            t1 = time.time()
            cov = inst.uv_coverage()
            t2 = time.time()
            t = timed(eng, lambda: inst.observe(sky), max(a.reps // 2, 3))
            print("%s observe, %2d hour angle(s): host set-up %.3f s, first uv_coverage (collapse, upload, kernels, sums) %.3f s, "
                  "%d samples in %d distinct; observe with the coverage cached %7.3f ms"
                  % (tag, nt, t1 - t0, t2 - t1, cov.n_samples, len(inst._collapsed()[0]), t * 1e3))
            del inst, cov, sky
        del box
        sys.stdout.flush()


if __name__ == "__main__":
    main()
