"""examples/example_cosmic_web.py runs at its smallest size: the volume and mass fractions of the four classes over a scan of
lambda_th, the mean delta per class, and P(k) of the filament mask."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_cosmic_web():
    spec = importlib.util.spec_from_file_location("example_cosmic_web", os.path.join(ROOT, "examples", "example_cosmic_web.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scan, cw, mean_delta, (k, pk_fil, pk_delta) = mod.main(32, smoothing=6.)
    assert scan.counts.shape == (9, 4) and np.all(scan.counts.sum(axis=1) == 32 ** 3) and scan.n_nan == 0
    np.testing.assert_allclose(scan.volume_fraction.sum(axis=1), 1., rtol=0, atol=1e-15)
    np.testing.assert_allclose(scan.mass_fraction.sum(axis=1), 1., rtol=0, atol=1e-14)
    # a higher threshold: more voids, fewer knots
    assert np.all(np.diff(scan.counts[:, 0]) >= 0) and np.all(np.diff(scan.counts[:, 3]) <= 0)
    # the scan's middle threshold is the single call's
    np.testing.assert_array_equal(scan.counts[4], cw.counts[0])
    assert np.all(np.isfinite(mean_delta)) and np.all(np.diff(mean_delta) > 0.)
    assert k.shape == pk_fil.shape == pk_delta.shape and np.any(pk_fil > 0.)
