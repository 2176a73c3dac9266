"""The reduced bispectrum Q of a Gaussian box and of the log-normal box made from it: the two have the same kind of P(k), and
only a third-order statistic tells them apart.  For a Gaussian field Q scatters around zero; the log-normal transform couples
the modes and Q is positive on every triangle.

    python examples/example_bispectrum.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                             # noqa: E402
from fastbox_amd import CosmoBox, default_cosmo                                # noqa: E402


def main(N=64):
    box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, realise_now=False, precision="f32", rng="device", seed=11)
    gauss = box.realise_density(inplace=False)
    lognormal = box.lognormal(gauss)
    kbins = np.linspace(0., (2. / 3.) * np.pi * N / box.Lx, 9)            # 8 shells, no triangle closes through an alias
    k, Bg, Qg, ntri = box.bispectrum(delta_x=gauss, kbins=kbins, reduced=True)
    k, Bl, Ql, ntri = box.bispectrum(delta_x=lognormal, kbins=kbins, reduced=True)
    ok = ntri > 0
    eq = ok & (np.abs(k[:, 0] - k[:, 2]) < 1e-12)                          # equilateral triples b1 = b2 = b3
    print("%d of %d triples have triangles (up to %.3g each)" % (np.count_nonzero(ok), ok.size, ntri.max()))
    print("   k1       k2       k3        ntri     Q Gaussian  Q log-normal")
    for t in np.nonzero(eq)[0]:
        print("%8.4f %8.4f %8.4f %10d %12.4f %12.4f" % (k[t, 0], k[t, 1], k[t, 2], ntri[t], Qg[t], Ql[t]))
    w = ntri[ok] / ntri[ok].sum()
    mg, ml = float(np.sum(w * Qg[ok])), float(np.sum(w * Ql[ok]))
    print("triangle-weighted mean Q: Gaussian %.4f, log-normal %.4f" % (mg, ml))
    return mg, ml


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64)
