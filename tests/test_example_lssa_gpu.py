"""examples/example_lssa.py runs on a small grid: the delay spectrum of the flagged cube is finite and follows the unflagged one."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_lssa():
    spec = importlib.util.spec_from_file_location("example_lssa", os.path.join(ROOT, "examples", "example_lssa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    full, holes, filled, w = mod.main(32)
    assert w.shape == (32, 32, 32) and (w == 0.).sum() > 3 * 32 * 32
    for sp in (full, holes, filled):
        assert sp.tau.shape == sp.ps_mean.shape == sp.ps_stderr.shape == (32,) and sp.n_los == 32 * 32
        assert np.all(np.isfinite(sp.ps_mean)) and np.all(np.isfinite(sp.ps_stderr)) and np.all(sp.ps_mean >= 0.)
    # the same sky: the total power of the flagged cube's spectrum stays within a factor of two of the unflagged one's
    ratio = holes.ps_mean.sum() / full.ps_mean.sum()
    assert 0.5 < ratio < 2., "total LSSA power of the flagged cube / unflagged: %.3f" % ratio
