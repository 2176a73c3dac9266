"""examples/example_minkowski.py runs at its smallest size: the functionals of a smoothed Gaussian and a smoothed log-normal
field beside the Gaussian expectations, and the per-channel Euler characteristic of a cube before and after pca_filter."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_minkowski():
    spec = importlib.util.spec_from_file_location("example_minkowski", os.path.join(ROOT, "examples", "example_minkowski.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    nu, (g, g_theory), (ln, ln_theory), v2 = mod.main(32, smoothing=6.)
    assert nu.shape == (13,) and v2.shape == (3, 32) and np.all(np.isfinite(v2))
    for mf in (g, ln):
        assert all(np.all(np.isfinite(v)) for v in (mf.v0, mf.v1, mf.v2, mf.v3))
        assert np.all(np.diff(mf.n3) <= 0) and np.all(mf.v1 >= 0.)
        np.testing.assert_array_equal(mf.euler, mf.n0 - mf.n1.sum(axis=0) + mf.n2.sum(axis=0) - mf.n3)
    # the volume fraction of the Gaussian field follows erfc; the log-normal field is skewed: less volume above the mean
    mid = nu.size // 2
    assert np.max(np.abs(g.v0 - g_theory[0])) < 0.05
    assert ln.v0[mid] < g.v0[mid] and ln.v0[mid] < 0.5
