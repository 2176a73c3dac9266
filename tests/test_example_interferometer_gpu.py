"""examples/example_interferometer.py runs on a small grid: the chromatic uv sampling of a hexagonal array throws the
foregrounds' k_par = 0 power up to k_par > 0, the more the larger k_perp."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_interferometer():
    spec = importlib.util.spec_from_file_location("example_interferometer", os.path.join(ROOT, "examples", "example_interferometer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    N = 32
    cyl, out, obs = mod.main(N)
    for name in ("sky", "dirty"):
        kperp, kpar, power, modes = cyl[name]
        assert power.shape == modes.shape == (3, N // 2 + 1) and np.all(modes > 0) and np.all(np.isfinite(power))
    cov = obs.coverage
    assert cov.empty_channels.size == 0 and np.all(cov.tot == 2 * cov.n_samples) and cov.n_samples == 91 * 90 // 2
    assert np.all(cov.ncell < N * N) and np.all(cov.ncell > 0)
    psf = obs.psf.host()
    assert np.allclose(psf[0, 0, :], 1., rtol=0, atol=1e-5) and np.max(np.abs(psf)) <= 1. + 1e-5
    sky, dirty = out["sky"][0], out["dirty"][0]
    # the sky's own k_par > 0 power is what a power law (and its slightly varying index) leaks over a finite band: below 2 %
    assert np.all(sky > 0) and np.all(sky < 0.02)
    # the instrument raises it on every scale, and by far the most where the baselines cross several cells over the band
    assert np.all(dirty > sky) and np.all(dirty[1:] > 5. * sky[1:]) and dirty[-1] > 10. * dirty[0]
    assert out["dirty"][1] > out["sky"][1]
