"""examples/example_fof_halos.py runs: COLA particles, friends-of-friends halos, the painted catalogue, the halo-matter
spectrum and the large-scale bias."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_fof_halos():
    spec = importlib.util.spec_from_file_location("example_fof_halos", os.path.join(ROOT, "examples", "example_fof_halos.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    halos, k, p_hm, p_mm, bias = mod.main(64)
    assert len(halos) > 50 and halos.count.min() >= 20 and np.all(np.diff(halos.count) <= 0)
    assert np.all(np.isfinite(p_hm)) and np.all(p_mm > 0)
    # halos of 20 particles or more (5e13 Msun here) are rarer than the matter and cluster more strongly: on the four largest
    # scales the cross spectrum is positive and above the matter's, by a factor well inside (1, 10)
    assert np.all(p_hm[:4] > p_mm[:4]) and 1. < bias < 10.
