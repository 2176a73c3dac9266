"""examples/example_cylindrical_power.py runs on a small grid: foregrounds pile power up at k_par = 0 and tie the channels
together, PCA cleaning removes both."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_cylindrical_power():
    spec = importlib.util.spec_from_file_location("example_cylindrical_power",
                                                  os.path.join(ROOT, "examples", "example_cylindrical_power.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cyl, maps = mod.main(32)
    for name in ("signal", "contaminated", "cleaned"):
        kperp, kpar, power, modes = cyl[name]
        assert power.shape == modes.shape == (4, 3) and np.all(modes > 0) and np.all(np.isfinite(power))
    # on the largest transverse scales the foregrounds (kelvins against a signal of 0.1 mK) dominate the k_par = 0 cell by
    # orders of magnitude; cleaning takes them out
    assert cyl["contaminated"][2][0, 0] > 1e3 * cyl["signal"][2][0, 0]
    assert cyl["cleaned"][2][0, 0] < 1e-3 * cyl["contaminated"][2][0, 0]
    off = ~np.eye(32, dtype=bool)
    before = mod.channel_coefficients(maps["contaminated"][1])
    after = mod.channel_coefficients(maps["cleaned"][1])
    assert before.shape == after.shape == (4, 32, 32)
    # foregrounds tie all channels together; removing 4 of 32 modes leaves a mean coefficient of about -4 / 28 plus scatter
    assert np.mean(before[0][off]) > 0.9 and np.all(np.abs([np.mean(x[off]) for x in after]) < 0.5)
