"""Measurement aid (GPU): the COLA particle mesh (fb_cola.hip) at 128^3, 256^3 and 512^3 in f32 and f64, timed with HIP events
on the box's stream.  Per size: ms for the 2LPT setup (fb_cola_lpt + fb_cola_init), ms per step (one force evaluation + one
kick/drift launch) and its split into

    paint   fb_cola_force without the force: CIC paint (fb_paint) and delta = count - 1
    r2c     fb_fft_r2c of delta (timed on its own, same buffers)
    3 c2r   the rest of fb_cola_force: three k-space multipliers and three fb_fft_c2r
    kick    fb_cola_kick: CIC readout of the force + kick + drift

(medians over --steps steps after one warm-up step), and the whole realise_density_cola call (default n_steps, velocities
included).  For per-launch times run one size per `rocprofv3 --kernel-trace --stats` run.

    python tools/cola_bench.py [--sizes 128,256,512] [--precs f32,f64] [--steps 5] [--no-call]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                             # noqa: E402
import torch                                                                   # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo, cola, _lib                   # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--precs", default="f32,f64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-call", action="store_true")
    a = ap.parse_args()
    for N in [int(x) for x in a.sizes.split(",")]:
        for prec in a.precs.split(","):
            stream = torch.cuda.current_stream().cuda_stream
            box = CosmoBox(cosmo=default_cosmo, box_scale=2. * N, nsamp=N, realise_now=False, precision=prec, rng="device",
                           seed=3, stream=stream or None)
            eng, P = box.engine, box.engine._plan
            d0 = box.realise_density(linear=True, redshift=0., inplace=False)
            ptr = d0.ptr
            g = cola.Growth(box.cosmo)
            tab = cola.launch_table(g, 0., 15., 16)
            st = eng.cola_buffers()
            S = eng.stream
            p = {k: v.ptr for k, v in st.items()}

            def setup():
                _lib.call("fb_cola_lpt", P, ptr, p["psi1"], p["psi2"], p["force"], p["h1"], p["h2"], S)
                _lib.call("fb_cola_init", P, p["psi1"], p["psi2"], float(tab[0]), float(tab[1]), p["pos"], p["pres"], S)
            timed(setup)
            t_setup = timed(setup)
            rows = []
            for j in range(a.steps + 1):
                row = np.ascontiguousarray(tab[3 + 6 * (j + 1): 9 + 6 * (j + 1)])
                t_paint = timed(lambda: _lib.call("fb_cola_force", P, p["pos"], p["count"], p["delta"], None, 0., None, None, S))
                t_r2c = timed(lambda: _lib.call("fb_fft_r2c", P, p["delta"], p["h1"], 0, S))
                t_force = timed(lambda: _lib.call("fb_cola_force", P, p["pos"], p["count"], p["delta"], p["force"],
                                                  float(tab[2]), p["h1"], p["h2"], S))
                t_kick = timed(lambda: _lib.call("fb_cola_kick", P, p["force"], p["psi1"], p["psi2"], p["pres"], p["pos"],
                                                 row.ctypes.data_as(_lib.P_double), 1, S))
                if j:
                    rows.append((t_force + t_kick, t_paint, t_r2c, t_force - t_paint - t_r2c, t_kick))
            med = np.median(np.array(rows), axis=0)
            res = dict(N=N, prec=prec, setup_ms=round(t_setup, 3), step_ms=round(med[0], 3), paint_ms=round(med[1], 3),
                       r2c_ms=round(med[2], 3), c2r3_ms=round(med[3], 3), kick_ms=round(med[4], 3))
            del st, p
            eng.sync()
            eng.release_idle_buffers()
            if not a.no_call:
                box.realise_density_cola(redshift=0.)
                eng.sync()
                eng.release_idle_buffers()
                res["call_ms_default_17_forces"] = round(timed(lambda: box.realise_density_cola(redshift=0.)), 1)
                eng.release_idle_buffers()
            print(json.dumps(res), flush=True)
            del box, eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
