"""examples/example_so_halos.py runs: COLA particles, friends-of-friends halos, spherical-overdensity radii and masses around
them, the two mass functions and the stacked density profile."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_so_halos():
    spec = importlib.util.spec_from_file_location("example_so_halos", os.path.join(ROOT, "examples", "example_so_halos.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fof, so, masses, n_fof, n_so, x, stack, used = mod.main(32)
    assert len(so) == len(fof) > 10 and set(np.unique(so.status)) <= {0, 1, 2}
    good = so.status == 0
    assert good.sum() > 5 and np.all(so.count[good] > 0) and np.all(so.count[~good] == 0) and np.all(np.isnan(so.radius[~good]))
    e = so.profiles.edges
    assert np.all(so.radius[good] > e[0]) and np.all(so.radius[good] < e[-1])
    np.testing.assert_allclose(so.mass[good], 4. * np.pi / 3. * 200. * so.rho_ref * so.radius[good] ** 3, rtol=1e-12)
    # R lies between two edges e_j <= R <= e_j+1 with N(< e_j) >= M(e_j) / m_p and N(< e_j+1) < M(e_j+1) / m_p, M(r) the
    # threshold mass inside r: the members inside R and M_200 / m_p both lie between those, a factor (e_j+1 / e_j)^3 apart
    step = (e[-1] / e[0]) ** (3. / (e.size - 1))
    ratio = so.count[good] * so.particle_mass / so.mass[good]
    assert np.all(ratio > 1. / (step * (1. + 1e-12))) and np.all(ratio < step * (1. + 1e-12))
    assert np.all(np.isfinite(so.sigma_v[good])) and np.all(so.sigma_v[good] >= 0.)
    assert np.all(np.diff(n_fof) <= 0) and np.all(np.diff(n_so) <= 0) and n_fof[0] > 0 and n_so[0] > 0
    assert used >= 1 and stack[0] > stack[-1] >= 0.
