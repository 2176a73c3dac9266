"""examples/example_three_point.py runs: COLA particles, friends-of-friends halos, the connected three-point multipoles of the
halos against randoms drawn on the device, and the pair-count xi(r) in the same bins."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_three_point():
    spec = importlib.util.spec_from_file_location("example_three_point", os.path.join(ROOT, "examples", "example_three_point.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fof, tp, xi = mod.main(32)
    assert tp.connected and tp.n_data == len(fof) > 10 and tp.n_random == 20 * len(fof) and tp.lmax == 4
    assert tp.zeta.shape == (5, 4, 4) and np.all(np.isfinite(tp.zeta)) and xi.shape == (4,)
    np.testing.assert_array_equal(tp.zeta, np.swapaxes(tp.zeta, 1, 2))
    assert tp.npairs.sum() > 0 and np.all(tp.npairs % 2 == 0)
