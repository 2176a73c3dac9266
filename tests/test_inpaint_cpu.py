"""The numpy statement of the constrained realisations (tests/inpaint_numpy.py) against vectors recorded from the reference's
fastbox/inpaint.py (tests/golden/inpaint_n16.npz, tools/make_golden_inpaint.py), and the host pieces of fastbox_amd.inpaint.
No GPU, no SciPy.

The bound on the statement is not fixed in advance: it is evaluated with np.linalg.solve and through eigh of A_p; that
deviation is delta_ref and the recorded realisations must lie within 10 delta_ref, floor 1e-12, relative to the largest
magnitude."""
import os

import numpy as np

from fastbox_amd import inpaint, rng
from tests import inpaint_numpy as inp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inpaint_n16.npz")
FLOOR = 1e-12


def reference_draws(seed, npix, realisations, n):
    """the reference's order: per pixel, per realisation, omega1 then omega2 -> (npix, realisations, 2, n)"""
    np.random.seed(int(seed))
    return np.random.randn(npix, realisations, 2, n)


def test_statement_reproduces_the_reference():
    g = np.load(GOLDEN)
    d, w, S, var, cr = g["d"], g["w"].astype(np.float64), g["S"], g["var"], g["cr"]
    assert cr.shape == (2, 256, 16) and (w[3] == 0).all() and (w[:, 11] == 0).all()
    om = reference_draws(g["seed"], 256, 2, 16)
    for i in range(2):
        a = inp.statement(d, w, S, var, om[:, i, 0], om[:, i, 1])
        b = inp.statement(d, w, S, var, om[:, i, 0], om[:, i, 1], via="eigh")
        big = np.max(np.abs(cr[i]))
        dref, dev = np.max(np.abs(a - b)) / big, np.max(np.abs(a - cr[i])) / big
        assert dev <= max(10. * dref, FLOOR), "realisation %d: deviation %.3e, delta_ref %.3e" % (i, dev, dref)


def test_simple_signal_cov_matches_the_recorded_values():
    g = np.load(GOLDEN)
    cov = inpaint.simple_signal_cov(g["cov_freqs"], float(g["cov_amplitude"]), float(g["cov_width"]), ridge_var=float(g["cov_ridge"]))
    dev = np.max(np.abs(cov - g["cov"]))
    assert dev <= 4 * 2. ** -53 * np.max(np.abs(g["cov"])), "deviation %.3e" % dev
    assert np.array_equal(inpaint.simple_signal_cov(np.arange(5.), 1., 2.), inp.simple_signal_cov(np.arange(5.), 1., 2.))


def test_gcr_normals_are_streams_7_to_9():
    N, seed, real = 6, 0x1234567890ABCDEF, 3
    for which in (1, 2, 3):
        got = rng.gcr_normals(N, which, seed, real)
        want = rng.stream_normals(N ** 3, 6 + which, seed, real)
        assert got.shape == (N * N, N) and got.dtype == np.float64
        assert np.array_equal(got.reshape(-1), want)
    assert not np.array_equal(rng.gcr_normals(N, 1, seed, real), rng.gcr_normals(N, 2, seed, real))
    assert not np.array_equal(rng.gcr_normals(N, 1, seed, real), rng.gcr_normals(N, 1, seed, real + 1))


def test_wiener_mean_returns_the_data_where_the_noise_is_small():
    """Nothing flagged and sigma -> small: s = S (S + sigma^2)^-1 d differs from d by at most sigma^2 |S^-1 d|_2 per line of
    sight.  A check of the statement, not of the device."""
    N, npix = 16, 8
    rs = np.random.RandomState(11)
    S = inp.simple_signal_cov(np.arange(N, dtype=np.float64), 1.0, 0.8, ridge_var=1e-3)          # cond ~ 1e3
    d = rs.standard_normal((npix, N)) @ inp.sqrt_psd(S).T
    var = np.full(N, 1e-10)
    s = inp.statement(d, np.ones((npix, N)), S, var)
    bound = 1e-10 * np.linalg.norm(np.linalg.solve(S, d.T), axis=0) * (1. + 1e-6)
    err = np.linalg.norm(s - d, axis=1)
    assert np.all(err <= bound + 1e-12), "largest |s - d| %.3e against %.3e" % (err.max(), bound.max())
    # and a fully flagged line of sight has the prior mean, 0
    assert np.array_equal(inp.statement(d[:1], np.zeros((1, N)), S, var), np.zeros((1, N)))
