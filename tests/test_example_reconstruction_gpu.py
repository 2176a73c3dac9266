"""examples/example_reconstruction.py runs at its smallest size: a COLA box, its reconstruction, r(k) with the linear field
before and after, xi(r) of both fields and the Landy-Szalay xi(r) of a moved subsample."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_reconstruction():
    spec = importlib.util.spec_from_file_location("example_reconstruction", os.path.join(ROOT, "examples", "example_reconstruction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    k, r_before, r_after, r, xi_before, xi_after, xi_ls = mod.main(32, subsample=4096)
    assert k.shape == r_before.shape == r_after.shape == (8,) and np.all(np.diff(k) > 0)
    assert all(np.all(np.isfinite(a)) for a in (r_before, r_after, xi_before, xi_after, xi_ls)) and xi_ls.shape == r.shape
    # non-linear evolution has decorrelated all but the largest scales from the linear field; moving the particles back by the
    # smoothed displacement restores part of it on every scale that had lost any
    lost = r_before < 0.95
    assert lost.sum() >= 5 and np.all(r_after[lost] > r_before[lost] + 0.05)
    assert r_before[0] > 0.95 and r_after[0] > 0.99 and np.all(np.abs(r_after) <= 1.)
