"""examples/example_halos.py runs: halo counts, catalogue, painting and the three spectra."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_halos():
    spec = importlib.util.spec_from_file_location("example_halos", os.path.join(ROOT, "examples", "example_halos.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    k, p_hh, p_dd, p_hd, nh = mod.main(32)
    good = ~np.isnan(p_dd)
    assert nh > 0 and np.all(np.isfinite(p_hh[good])) and np.all(np.isfinite(p_hd[good]))
    # on large scales the halos trace the matter (bias 1): the cross spectrum is positive and of the matter's size
    assert np.all(p_hd[good][:3] > 0) and np.all(np.abs(p_hd[good][:3] / p_dd[good][:3] - 1.) < 0.5)
