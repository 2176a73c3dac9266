"""CPU: host model of the halo streams (fastbox_amd/rng.py), the numpy catalogue order against the reference's golden
catalogues, and the C ABI of the halo entry points."""
import math
import os

import numpy as np
import pytest

from fastbox_amd import rng
from tests import halos_numpy as hn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_stream5_known_answers():
    u = rng.poisson_uniforms(4, 12345, 7)
    np.testing.assert_array_equal(u, [0.13285211889233667, 0.10338643381723561, 0.7135018474796646, 0.08708773662965502])
    assert np.all((u > 0) & (u < 1))
    np.testing.assert_array_equal(rng.stream_poisson(np.array([0.5, 3., 30., 1e4]), 12345, 7), [0, 1, 33, 9864])
    # voxel i of a box is call i: a later window of the stream is the same numbers
    np.testing.assert_array_equal(rng.poisson_uniforms(3, 12345, 7, first=1), u[1:])


def test_stream6_known_answers():
    s = rng.scatter_uniforms(2, 12345, 7)
    np.testing.assert_array_equal(s, [[0.8078856212789137, 0.3139635705192031, 0.7424996248702247],
                                      [0.8427082222900253, 0.8739856436063074, 0.14909443179993956]])
    big = rng.scatter_uniforms(20000, 3, 0)
    assert big.min() >= 0. and big.max() < 1. - 1e-8


@pytest.mark.parametrize("lam", [0.01, 0.5, 3., 30., 300., 1e4])
def test_poisson_sampler_chi2(lam):
    n = 200000
    k = rng.poisson_inverse(np.full(n, lam), rng.poisson_uniforms(n, 2024, int(lam * 100)))
    lo, hi = int(max(0, math.floor(lam - 6 * math.sqrt(lam) - 3))), int(math.ceil(lam + 6 * math.sqrt(lam) + 6))
    ks = np.arange(lo, hi + 1)
    pmf = np.exp(ks * math.log(lam) - lam - np.array([math.lgamma(x + 1.) for x in ks]))
    exp_ = n * pmf
    obs = np.array([(k == x).sum() for x in ks], dtype=np.float64)
    assert obs.sum() >= n - 2                   # nothing outside +-6 sigma but by chance
    keep = exp_ >= 5.                          # pool the tails into the neighbouring classes
    e = np.concatenate([[exp_[:np.argmax(keep)].sum() + exp_[np.argmax(keep)]], exp_[keep][1:]])
    o = np.concatenate([[obs[:np.argmax(keep)].sum() + obs[np.argmax(keep)]], obs[keep][1:]])
    last = np.nonzero(keep)[0][-1]
    e[-1] += exp_[last + 1:].sum()
    o[-1] += obs[last + 1:].sum()
    dof = max(len(e) - 1, 1)
    chi2 = float(((o - e) ** 2 / e).sum())
    assert chi2 < dof + 6 * math.sqrt(2 * dof) + 10, (chi2, dof)
    assert abs(k.mean() - lam) < 6 * math.sqrt(lam / n) + 1e-12


def test_poisson_inverse_edges():
    out = rng.poisson_inverse(np.array([0., -1., np.nan, 1e-300, 5.]), np.array([0.5, 0.5, 0.5, 0.999, 1e-300]))
    np.testing.assert_array_equal(out, [0, 0, 0, 0, 0])


@pytest.mark.parametrize("N", [16, 32])
def test_catalogue_order_matches_golden(N):
    g = np.load(os.path.join(GOLDEN, "halos_n%d.npz" % N))
    np.testing.assert_array_equal(hn.catalogue(g["counts"], g["L"]), g["cat"])
    np.random.seed(int(g["seed_cat"]))
    nh = int(g["counts"].sum())
    u = np.random.uniform(0., 1. - 1e-8, 3 * nh).reshape(nh, 3)
    np.testing.assert_array_equal(hn.catalogue(g["counts"], g["L"], u), g["cat_scatter"])


def test_expected_counts_oracle_reproduces_golden_draw():
    g = np.load(os.path.join(GOLDEN, "halos_n16.npz"))
    lam = hn.expected_counts(g["delta"].astype(np.float64), g["nbar_z"], g["bias"], g["L"])
    np.random.seed(int(g["seed_counts"]))
    np.testing.assert_array_equal(np.random.poisson(lam=lam), g["counts"])


def test_paint_oracle_conserves_weight():
    rs = np.random.RandomState(3)
    pos = rs.uniform(-50., 150., (500, 3))
    w = rs.uniform(0.5, 2., 500)
    for win in ("ngp", "cic", "tsc"):
        m = hn.paint(pos, 8, (100., 100., 100.), win, w)
        assert abs(m.sum() - w.sum()) < 1e-10 * w.sum()


def test_halo_abi_symbols_exported():
    from fastbox_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load()
    for name in ("fb_halo_lambda", "fb_halo_counts", "fb_halo_catalogue_size", "fb_halo_catalogue", "fb_paint",
                 "fb_paint_compensate"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.fb_version() == 102


def test_construct_bins_not_implemented():
    from fastbox_amd.halos import HaloDistribution
    with pytest.raises(NotImplementedError):
        HaloDistribution(None, (1e12, 1e15), 10).construct_bins(0.5)
