"""CPU: the host models of the rng='device' sky draws (fastbox_amd/rng.py: streams 2, 3, 4) and the numpy statements
tests/test_sky_kernels_gpu.py compares the sky kernels with (tests/sky_numpy.py).  The statements must agree with each
other, and the f32 / f64 host models must differ by a finite, non-zero amount, before anything is compared on a GPU."""
import types

import numpy as np
import pytest
import scipy.ndimage

from fastbox_amd import rng, sky
from oracle import sky_oracle as so
from tests import sky_numpy as sn


def test_sky_draw_seed_is_what_the_models_hand_to_the_library():
    box = types.SimpleNamespace(seed=4, engine=None, N=16)
    m = sky._Maps(box)
    want = [(4 * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * n) & (2 ** 64 - 1) for n in (1, 2, 3)]
    assert [m.next_seed() for _ in range(3)] == want
    assert [sky.sky_draw_seed(4, n) for n in (1, 2, 3)] == want
    assert len({sky.sky_draw_seed(s, n) for s in (0, 1, 2 ** 63) for n in (1, 2)}) == 6
    assert 0 <= sky.sky_draw_seed(2 ** 64 - 1, 2 ** 40) < 2 ** 64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [16, 18])
def test_sky_draws_are_the_stated_slices_of_their_streams(N, dtype):
    seed = sky.sky_draw_seed(9, 1)
    re, im = rng.sky_map_noise(N, seed, dtype)
    s2 = rng.stream_normals(2 * N * N, 2, seed, 0, dtype)
    assert re.shape == im.shape == (N, N) and re.dtype == np.dtype(dtype)
    assert np.array_equal(re.ravel(), s2[0::2]) and np.array_equal(im.ravel(), s2[1::2])
    # element q: call q >> 1, words (0, 1) for even q and (2, 3) for odd q
    q = np.arange(N * N, dtype=np.uint64)
    o = rng._call(q >> np.uint64(1), 2, seed, 0)
    odd = (q & np.uint64(1)).astype(bool)
    g0, g1 = rng.box_muller(np.where(odd, o[2], o[0]), np.where(odd, o[3], o[1]), dtype)
    assert np.array_equal(re.ravel(), g0) and np.array_equal(im.ravel(), g1)
    idx = rng.sky_index_noise(N, seed, dtype)
    assert idx.shape == (N, N) and np.array_equal(idx.ravel(), rng.stream_normals(N * N, 3, seed, 0, dtype))
    cube = rng.sky_noise_normals(N, seed, dtype)
    assert cube.shape == (N, N, N) and np.array_equal(cube.ravel(), rng.stream_normals(N ** 3, 4, seed, 0, dtype))
    # call c of stream 4 supplies the flat elements 4 c .. 4 c + 3: at N = 18 call 4 straddles two lines of sight
    o = rng._call(np.uint64(4), 4, seed, 0)
    g = np.concatenate([np.ravel(x) for x in rng.box_muller(o[0], o[1], dtype) + rng.box_muller(o[2], o[3], dtype)])
    assert np.array_equal(cube.ravel()[16:20], g)


def test_sky_draws_have_unit_variance_and_differ_per_seed_and_stream():
    N, seed = 24, sky.sky_draw_seed(3, 1)
    re, im = rng.sky_map_noise(N, seed)
    idx = rng.sky_index_noise(N, seed)
    cube = rng.sky_noise_normals(N, seed)
    for a in (re, im, idx, cube):
        n = a.size
        assert abs(a.mean()) < 5 / np.sqrt(n) and abs(a.var() - 1) < 5 * np.sqrt(2. / n)
    assert abs(np.mean(re * im)) < 5 / np.sqrt(N * N)
    flat = [re.ravel(), im.ravel(), idx.ravel(), cube.ravel()[:N * N]]
    for i in range(4):
        for j in range(i):
            assert abs(np.corrcoef(flat[i], flat[j])[0, 1]) < 5 / np.sqrt(N * N)
    other = sky.sky_draw_seed(3, 2)
    assert abs(np.corrcoef(cube.ravel(), rng.sky_noise_normals(N, other).ravel())[0, 1]) < 5 / np.sqrt(N ** 3)
    assert abs(np.corrcoef(idx.ravel(), rng.sky_index_noise(N, other).ravel())[0, 1]) < 5 / np.sqrt(N * N)
    assert abs(np.corrcoef(re.ravel(), rng.sky_map_noise(N, other)[0].ravel())[0, 1]) < 5 / np.sqrt(N * N)
    assert np.array_equal(cube, rng.sky_noise_normals(N, seed))


@pytest.mark.parametrize("N", sn.SIZES)
def test_f32_and_f64_models_of_the_draws_differ_by_a_finite_amount(N):
    seed = sky.sky_draw_seed(4, 1)
    sigma = np.linspace(0.5, 2., N)
    d = np.max(np.abs(sn.noise_cube_model(N, seed, sigma, np.float32) - sn.noise_cube_model(N, seed, sigma, np.float64)))
    assert np.isfinite(d) and 0 < d < 1e-3, d
    d = np.max(np.abs(sn.index_map_model(N, seed, 2.07, 0.05, np.float32) - sn.index_map_model(N, seed, 2.07, 0.05, np.float64)))
    assert np.isfinite(d) and 0 < d < 1e-5, d
    geo = {"N": N, "Lx": 2e3, "Ly": 1.5e3}
    maps = [sn.foreground_model(geo, 1900., 57., 1.1, 10., 3., N, seed, dt) for dt in (np.float32, np.float64)]
    d = np.max(np.abs(maps[0] - maps[1])) / np.max(np.abs(maps[1] - 10.))
    assert np.isfinite(d) and 0 < d < 1e-4, d


@pytest.mark.parametrize("N", [16, 18, 30])
def test_the_two_smoothing_statements_agree(N):
    """The double loop of tests/sky_numpy.py against scipy.ndimage.gaussian_filter(mode='wrap'), where scipy takes the
    radius (r < N), on the maps of the GPU test; and the spike rows are periodic shifts of the folded weights."""
    maps = sn.smoothing_maps(N)
    for r in sn.smoothing_radii(N):
        w = sn.weights_for_radius(r)
        out = {k: sn.wrap_smooth(v, w, r) for k, v in maps.items()}
        if 1 <= r < N:
            for k, v in maps.items():
                ref = scipy.ndimage.gaussian_filter(v, sigma=r / 4., mode="wrap")
                assert np.max(np.abs(out[k] - ref)) < 1e-14, (r, k)
        if r == 0:
            assert all(np.array_equal(out[k], maps[k]) for k in maps)
        W0, W1 = sn.folded_weights(w, r, N), sn.folded_weights(w, r, N, at=N - 1)
        assert np.array_equal(W1, np.roll(W0, -1)) and abs(W0.sum() - 1) < 1e-14
        assert np.max(np.abs(out["spike00"] - np.outer(W0, W0))) < 1e-15
        assert np.array_equal(out["spikeNN"], np.roll(out["spike00"], (-1, -1), axis=(0, 1)))
        if 2 * r + 1 <= N:          # one term per output: exact
            assert np.array_equal(out["spike00"], np.outer(W0, W0))
            assert np.array_equal(W0, np.roll(np.concatenate([w, np.zeros(N - 2 * r - 1)]), -r))


@pytest.mark.parametrize("N", [16, 30])
def test_the_f32_statement_of_the_foreground_cube_against_the_f64_one(N):
    amps, alpha = sn.cube_inputs(N)
    assert alpha.min() == -3.5 and alpha.max() == 3.5 and (amps == 0).sum() == 1 and (amps < 0).sum() == 2
    freqs = np.linspace(900., 700., N)
    a32, al32 = sn.as_stored(amps, "f32"), sn.as_stored(alpha, "f32")
    for idx, idx32 in ((alpha, al32), (-2.7, -2.7), (3.5, 3.5)):
        want = so.construct_cube(a32, idx32, freqs)
        rel = sn.relative_per_channel(sn.fg_cube_f32(amps, idx, freqs / 130.), want)
        assert rel.shape == (N,) and np.all(np.isfinite(rel)) and np.all(rel > 0) and np.all(rel < 2e-6), rel.max()
        assert np.all(np.signbit(want[1, 2])) and np.all(want[0, 0] == 0) and np.all(want[N - 1, N - 1] > 0)
