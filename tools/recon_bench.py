"""Measurement aid (GPU): the stages of CosmoBox.reconstruct for the 256^3 particles of a COLA run (z = 0, 2 Mpc spacing) and
for the friends-of-friends halo catalogue of the same run, timed with HIP events on the box's stream (median of --reps calls
after one warm-up; everything already on the device), each beside its byte model over 8 TB/s:

    density      fb_paint (CIC) and delta = n / nbar - 1                 no model: atomics
    r2c          delta -> delta(k)                                        real + half
    displacement fb_recon_displacement: one multiplier pass, three c2r    (1 + 3) half, then 3 (half + real)
    shift        fb_recon_shift, particles in COLA order and shuffled     48 n + the three fields once + the interleaved copy
                 (from N^3 / 8 particles on it gathers from an            (3 reals read, 4 written per node)
                 interleaved copy staged in the call; the halos do not)
    kick         fb_cola_kick's drift launch on the same particles        the yardstick: the same 8 x 3 gather, particle-ordered
    readout      fb_mesh_readout of the three fields                      48 n + the three fields once
    randoms      fb_uniform_positions (4 n) and fb_grid_positions         24 n written

and the whole call, host clock round ``box.reconstruct`` with 'grid' randoms and with 4 n drawn ones.  --host-size S: the numpy
statement of the same pipeline (tests/recon_numpy.py) for S^3 particles on an S^3 grid, one core, no GPU needed.

    python tools/recon_bench.py [--precs f32,f64] [--reps 5] [--size 256] [--host-size 0]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402

PEAK = 8e12                                                                    # bytes per second (spec)


def host(S):
    from tests import recon_cases as rc, recon_numpy as rn
    L = (2. * S,) * 3
    rs = np.random.RandomState(1)
    data = rn.wrap(rn.grid_positions(S, L) + rs.normal(scale=2., size=(S ** 3, 3)), L)
    t0 = time.time()
    rn.reconstruct(data, rn.grid_positions(S, L), S, L, 10.)
    return dict(what="host", particles="%d^3" % S, grid="%d^3" % S, randoms="grid", numpy_ms=round(1e3 * (time.time() - t0), 1))


def device(N, prec, reps):
    import torch
    from fastbox_amd import CosmoBox, default_cosmo, _lib, recon
    from fastbox_amd.halos import HaloCatalogue

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median_ms(fn):
        timed(fn)
        return float(np.median([timed(fn) for _ in range(reps)]))

    def wall_ms(fn):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    stream = torch.cuda.current_stream().cuda_stream
    box = CosmoBox(cosmo=default_cosmo, box_scale=2. * N, nsamp=N, realise_now=False, precision=prec, rng="device", seed=3,
                   stream=stream or None)
    eng = box.engine
    real, half = float(eng.nbytes["real"]), float(eng.nbytes["half"])
    _, parts = box.realise_density_cola(redshift=0., keep_velocities=False, seed=12, return_particles=True, inplace=False)
    halos = box.find_halos(parts)
    eng.release_idle_buffers()
    n = parts.n
    rows = []

    def row(stage, ms, model_bytes=None, **kw):
        d = dict(what=stage, prec=prec, ms=round(ms, 3))
        if model_bytes is not None:
            d["model_ms"] = round(1e3 * model_bytes / PEAK, 3)
        d.update(kw)
        rows.append(d)
        print(json.dumps(d), flush=True)

    call = _lib.call
    mesh, delta = eng.empty("real"), eng.empty("real")
    row("density", median_ms(lambda: (call("fb_paint", eng._plan, parts.ptr, None, n, 1, mesh.ptr, eng.stream),
                                      call("fb_real_axpby", eng._plan, mesh.ptr, None, delta.ptr, 1., 0., -1., eng.stream))),
        particles="%d^3" % N)
    hk = eng.empty("half")
    row("r2c", median_ms(lambda: call("fb_fft_r2c", eng._plan, delta.ptr, hk.ptr, 0, eng.stream)), real + half)
    work, psi = eng._alloc_bytes(3 * eng.nbytes["half"]), eng._alloc_bytes(3 * eng.nbytes["real"])
    row("displacement", median_ms(lambda: call("fb_recon_displacement", eng._plan, hk.ptr, work.ptr, psi.ptr, 10., 1., 0.5, eng.stream)),
        4 * half + 3 * (half + real))

    shuffled = HaloCatalogue(eng, eng.upload_raw(np.asarray(parts)[np.random.RandomState(5).permutation(n)]), n)
    eng.sync()
    out = eng._alloc_bytes(24 * n)
    gather_model = 48. * n + 3 * real
    for name, cat in (("COLA order", parts), ("shuffled", shuffled)):
        row("shift", median_ms(lambda: call("fb_recon_shift", eng._plan, psi.ptr, cat.ptr, n, 1, 1., 0.5, out.ptr, eng.stream)),
            gather_model + 7 * real, particles=name, layout="interleaved copy, staged in the call")
        vals = eng._alloc_bytes(24 * n)
        row("readout", median_ms(lambda: call("fb_mesh_readout", eng._plan, psi.ptr, 3, cat.ptr, n, 1, vals.ptr, eng.stream)),
            gather_model, particles=name)
        del vals
    # the yardstick: the drift launch of the COLA kick on the same particles, the displacement as its force
    zero = eng._alloc_bytes(3 * eng.nbytes["real"])
    pres = eng._alloc_bytes(3 * eng.nbytes["real"])
    z = torch.zeros(3 * N ** 3, dtype=torch.float32 if prec == "f32" else torch.float64, device="cuda")
    for b in (zero, pres):
        call("fb_memcpy_d2d", b.ptr, z.data_ptr(), 3 * eng.nbytes["real"], eng.stream)
    coef = (ctypes.c_double * 6)(1e-3, 0., 0., 1e-3, 0., 0.)
    for name, cat in (("COLA order", parts), ("shuffled", shuffled)):
        call("fb_memcpy_d2d", out.ptr, cat.ptr, 24 * n, eng.stream)
        row("kick", median_ms(lambda: call("fb_cola_kick", eng._plan, psi.ptr, zero.ptr, zero.ptr, pres.ptr, out.ptr, coef, 1, eng.stream)),
            48. * n + 3 * real + 4 * 3 * real, particles=name)
    del zero, pres, z, out, shuffled
    torch.cuda.empty_cache()
    eng.release_idle_buffers()

    rnd = eng._alloc_bytes(24 * 4 * n)
    row("randoms", median_ms(lambda: call("fb_uniform_positions", eng._plan, 3, 0, 4 * n, rnd.ptr, eng.stream)), 24. * 4 * n, n="4 x %d^3" % N)
    row("randoms", median_ms(lambda: call("fb_grid_positions", eng._plan, rnd.ptr, eng.stream)), 24. * n, n="grid %d^3" % N)
    row("shift", median_ms(lambda: call("fb_recon_shift", eng._plan, psi.ptr, rnd.ptr, n, 1, 1., 0.5, rnd.ptr, eng.stream)),
        gather_model + 7 * real, particles="grid randoms, in place", layout="interleaved copy, staged in the call")
    hb = eng._alloc_bytes(24 * halos.n)
    row("shift", median_ms(lambda: call("fb_recon_shift", eng._plan, psi.ptr, halos.ptr, halos.n, 1, 1., 0.5, hb.ptr, eng.stream)),
        particles="%d halos" % halos.n, layout="component-major")
    del hb
    del rnd, work, psi, hk, mesh, delta
    eng.release_idle_buffers()

    row("reconstruct", wall_ms(lambda: box.reconstruct(parts, randoms='grid', smoothing=10., f=0.5)), particles="%d^3" % N, randoms="grid",
        clock="host")
    row("reconstruct", wall_ms(lambda: box.reconstruct(parts, smoothing=10., f=0.5)), particles="%d^3" % N, randoms="4 n drawn", clock="host")
    dm = recon.density_contrast(box, parts)
    row("reconstruct", wall_ms(lambda: box.reconstruct(halos, delta=dm, smoothing=10., f=0.5)), particles="%d halos" % halos.n,
        randoms="4 n drawn", delta="the matter density", clock="host")
    psi3 = recon.displacement(box, dm, 10., 1., 0.5)
    row("readout", wall_ms(lambda: box.readout(list(psi3), halos)), particles="%d halos" % halos.n, clock="host")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--host-size", type=int, default=0, help="S: time the numpy statement at S^3 on the host (0: not)")
    a = ap.parse_args()
    for prec in [x for x in a.precs.split(",") if x]:
        device(a.size, prec, a.reps)
    if a.host_size:
        print(json.dumps(host(a.host_size)), flush=True)


if __name__ == "__main__":
    main()
