"""Golden vectors of the reference's fastbox/inpaint.py (gaussian_cr_1d, simple_signal_cov) for tests/test_inpaint_*.py.  Loads
the reference module by path (it needs only numpy and SciPy), so it runs only where the reference sources are present; the
output is committed under tests/golden/.

    python tools/make_golden_inpaint.py <path of the reference's fastbox/inpaint.py>

inpaint_n16.npz holds a 16^3 case seen as (256, 16): d, w (0/1 flags; one line of sight fully flagged, one channel flagged in
every pixel), S, var (the diagonal of the noise covariance), seed (the np.random.seed value set before the call) and cr (the
real part of realisations=2 with add_noise=False, shape (2, 256, 16)); and cov_freqs, cov_amplitude, cov_width, cov_ridge, cov
for simple_signal_cov.  cg_maxiter is passed as an int: recent SciPy rejects the reference's float default."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_inpaint(path):
    spec = importlib.util.spec_from_file_location("reference_inpaint", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(mod, N=16, seed=20240607):
    npix = N * N
    freqs = np.arange(N, dtype=np.float64)
    S = mod.simple_signal_cov(freqs, 1.0, N / 12., ridge_var=1e-10)
    var = np.full(N, 1e-2)
    rs = np.random.RandomState(7)
    lam, V = np.linalg.eigh(S)
    d = (rs.standard_normal((npix, N)) * np.sqrt(np.maximum(lam, 0.))) @ V.T + np.sqrt(var) * rs.standard_normal((npix, N))
    w = np.ones((npix, N))
    w[:, 11] = 0.                                      # a channel flagged in every pixel
    w[1, 3] = 0.                                       # one more flagged channel
    w[2, 5:9] = 0.                                     # a run
    w[3, :] = 0.                                       # a fully flagged line of sight
    w[rs.uniform(size=(npix, N)) < 0.05] = 0.          # and 5 % at random (pixel 0 is restored below)
    w[0, :] = 1.
    w[0, 11] = 0.
    np.random.seed(seed)
    cr = mod.gaussian_cr_1d(d, w, S, np.diag(var), realisations=2, add_noise=False, precondition=True, cg_maxiter=10000,
                            verbose=False)
    assert np.max(np.abs(cr.imag)) == 0.
    cf = np.linspace(400., 410., 7)
    return dict(d=d, w=w.astype(np.int8), S=S, var=var, seed=np.int64(seed), cr=cr.real,
                cov_freqs=cf, cov_amplitude=np.float64(2.5), cov_width=np.float64(3.0), cov_ridge=np.float64(1e-8),
                cov=mod.simple_signal_cov(cf, 2.5, 3.0, ridge_var=1e-8))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = load_inpaint(sys.argv[1])
    out = os.path.join(ROOT, "tests", "golden", "inpaint_n16.npz")
    np.savez_compressed(out, **make(mod))
    print("wrote", out)


if __name__ == "__main__":
    main()
