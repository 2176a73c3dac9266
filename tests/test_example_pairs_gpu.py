"""examples/example_pair_correlation.py runs: COLA particles, friends-of-friends halos, and the halo auto-, halo-matter and
matter correlation functions by pair counts."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_pair_correlation():
    spec = importlib.util.spec_from_file_location("example_pair_correlation", os.path.join(ROOT, "examples", "example_pair_correlation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    halos, hh, hm, mm = mod.main(64)
    for p in (hh, hm, mm):
        assert np.all(np.isfinite(p.npairs)) and np.all(p.npairs >= 0) and p.npairs.sum() > 0
    assert hh.auto and mm.auto and not hm.auto
    assert np.all(hh.npairs % 2 == 0) and np.all(mm.npairs % 2 == 0)                # ordered pairs: every unordered one twice
    # halos of 20 particles or more are rarer than the matter and cluster more strongly
    print("xi_hh", hh.xi[-3:], "xi_mm", mm.xi[-3:])
    assert np.all(hh.xi[-3:] > mm.xi[-3:])
