"""examples/example_void_detection.py runs, and the reference's per-region loop on the host accepts the regions the device's
region means accept."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_void_detection_literal_and_device_idioms_agree():
    spec = importlib.util.spec_from_file_location("example_void_detection",
                                                  os.path.join(ROOT, "examples", "example_void_detection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a, b = mod.main(32, literal=True), mod.main(32, literal=False)
    assert b.size > 0
    np.testing.assert_array_equal(a, b)
