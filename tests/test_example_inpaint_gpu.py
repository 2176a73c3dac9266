"""examples/example_inpaint.py runs on a small grid: the in-painted cube keeps the data and fills every hole."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_inpaint():
    spec = importlib.util.spec_from_file_location("example_inpaint", os.path.join(ROOT, "examples", "example_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    painted, mean_filled, w = mod.main(32)
    assert painted.shape == mean_filled.shape == w.shape == (32, 32, 32)
    assert (w == 0.).sum() > 2 * 32 * 32
    assert np.all(np.isfinite(painted)) and np.all(np.isfinite(mean_filled))
