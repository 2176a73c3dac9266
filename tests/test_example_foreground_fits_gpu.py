"""examples/example_foreground_fits.py runs on a small grid: every residual is finite where it is not flagged (and exactly 0
under the flags the two fits honour), and every fitted cleaner leaves less power than the uncleaned cube holds."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_foreground_fits():
    spec = importlib.util.spec_from_file_location("example_foreground_fits", os.path.join(ROOT, "examples", "example_foreground_fits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    residuals, w, ratios = mod.main(32)
    assert set(residuals) == {"uncleaned", "pca_filter", "polynomial_filter", "run_fit", "gpr_filter"}
    assert w.shape == (32,) and (w == 0.).sum() == 3
    for name, cube in residuals.items():
        assert cube.shape == (32, 32, 32)
        assert np.all(np.isfinite(cube[:, :, w != 0.])), "%s: %d values are not finite" % (name, int((~np.isfinite(cube)).sum()))
    for name in ("polynomial_filter", "run_fit"):
        assert np.all(residuals[name][:, :, w == 0.] == 0.)
    for name in ("polynomial_filter", "run_fit", "gpr_filter"):
        assert np.all(ratios[name] < ratios["uncleaned"]), "%s: residual power / uncleaned power %s" % (name, ratios[name] / ratios["uncleaned"])
