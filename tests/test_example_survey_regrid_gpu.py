"""examples/example_survey_regrid.py runs on a small grid: the regridded cube and the binned halos of one box correlate."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_example_survey_regrid():
    spec = importlib.util.spec_from_file_location("example_survey_regrid", os.path.join(ROOT, "examples", "example_survey_regrid.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    k, p_x, p_dd = ex.main(32)
    assert k.shape == p_x.shape == p_dd.shape and k.size >= 8 and np.all(np.isfinite(p_x)) and np.all(np.isfinite(p_dd))
    # unit-bias halos of the box against the box's own density seen at half resolution: positive on the largest scales, and no
    # larger than the matter power itself by more than the shot noise and the scatter of a few modes allow
    assert np.all(p_x[:3] > 0.) and np.all(p_x[:3] < 2. * p_dd[:3])
