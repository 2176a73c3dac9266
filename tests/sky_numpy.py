"""TEST INFRASTRUCTURE ONLY.  Plain numpy statements of what the sky kernels (fb_field_kernels.h, k_sky_*) compute, on the
inputs the tests construct, and the host models of the rng='device' sky draws built from fastbox_amd/rng.py.  Shared by
tests/test_sky_draws_cpu.py (which checks that the statements agree with each other, no GPU) and
tests/test_sky_kernels_gpu.py (which checks the device against them)."""
import numpy as np

from fastbox_amd import rng as hostrng
from oracle import sky_oracle as so

U32 = 2.0 ** -24                 # unit round-off of float32
SIZES = (16, 18, 24, 30, 72)     # golden size; N % 4 = 2; not a power of two; N % 4 = 2 with a factor 5; two trips of a 64-thread block
CUBOID = (2e3, 1.5e3, 1e3)
RADIOMETER = dict(Tinst=18., tp=2., fov=1., Ndish=64)


def as_stored(a, precision):
    """The values of `a` as a plan of that precision holds them, in float64."""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if precision == "f32" else a


class ReplayNormals(object):
    """Stands in for np.random in the oracle: hands out prepared arrays, one per normal() call, in order."""

    def __init__(self, *arrays):
        self.arrays = list(arrays)

    def normal(self, mu, sigma, shape):
        a = self.arrays.pop(0)
        assert a.shape == tuple(shape)
        return mu + sigma * np.asarray(a, dtype=np.float64)


# ---- Gaussian smoothing ------------------------------------------------------------------------------------------------
def wrap_correlate_axis(a, w, r, axis):
    """out[i] = sum_j w[j] in[(i + j - r) mod N] along `axis`: the plain double loop in float64, j ascending."""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    N = a.shape[0]
    out = np.zeros_like(a)
    for i in range(N):
        for j in range(2 * r + 1):
            out[i] += w[j] * a[(i + j - r) % N]
    return np.moveaxis(out, 0, axis)


def wrap_smooth(a, w, r, precision="f64"):
    """Axis 0, then axis 1, as fb_sky_gaussian_filter; an f32 plan stores the map between and after the passes."""
    t = as_stored(wrap_correlate_axis(a, w, r, 0), precision)
    return as_stored(wrap_correlate_axis(t, w, r, 1), precision)


def folded_weights(w, r, N, at=0):
    """Response of one pass to a unit spike at index `at`: W[i] = sum of w[j] over j = r - i + at (mod N), j ascending."""
    W = np.zeros(N)
    for j in range(2 * r + 1):
        W[(r - j + at) % N] += w[j]
    return W


def weights_for_radius(r):
    """The weights scipy forms for the sigma whose truncated radius is r (r = 0: sigma 0.1, the identity)."""
    w, radius = so.gaussian_weights(0.1 if r == 0 else r / 4.)
    assert radius == r and w.size == 2 * r + 1
    return np.ascontiguousarray(w)


def smoothing_radii(N):
    return (0, 1, N // 2, N - 1, N, 2 * N + 3)


def smoothing_maps(N):
    """name -> (N, N) map: a spike at (0, 0), one at (N-1, N-1), a random map."""
    a = np.zeros((N, N)); a[0, 0] = 1.
    b = np.zeros((N, N)); b[N - 1, N - 1] = 1.
    return {"spike00": a, "spikeNN": b, "random": np.random.RandomState(100 + N).normal(size=(N, N))}


# ---- foreground cube ---------------------------------------------------------------------------------------------------
def cube_inputs(N):
    """Amplitudes with a 0, a negative value and 1e-30 planted; spectral indices spanning -3.5 .. +3.5."""
    rs = np.random.RandomState(200 + N)
    amps = rs.uniform(1., 100., size=(N, N))
    amps[0, 0], amps[1, 2], amps[N - 1, N - 1], amps[N - 1, 0] = 0., -7.5, 1e-30, -1e-30
    alpha = rs.permutation(np.linspace(-3.5, 3.5, N * N)).reshape(N, N)
    return amps, alpha


def fg_cube_f32(amps, spectral_idx, ratio):
    """k_sky_fg_cube's single-precision expression, a * exp2f(float(alpha) * float(log2 ratio)), in numpy float32."""
    a = np.asarray(amps).astype(np.float32)
    lr = np.log2(np.asarray(ratio, dtype=np.float64)).astype(np.float32)
    al = np.float32(spectral_idx) if np.isscalar(spectral_idx) else np.asarray(spectral_idx).astype(np.float32)[:, :, None]
    x = al * lr[None, None, :]
    assert x.dtype == np.float32
    out = a[:, :, None] * np.exp2(x)
    assert out.dtype == np.float32
    return out.astype(np.float64)


def relative_per_channel(got, want):
    """max over the pixels of |got - want| / |want| for every channel (pixels with want = 0 must match exactly)."""
    z = want == 0
    assert np.array_equal(got[z], want[z])
    with np.errstate(all="ignore"):
        rel = np.where(z, 0., np.abs(got - want) / np.abs(want))
    return rel.reshape(-1, want.shape[-1]).max(axis=0)


# ---- host models of the rng='device' draws ----------------------------------------------------------------------------
def noise_cube_model(N, seed, sigma, dtype):
    """k_sky_noise_cube with the device generator: (T)(double(g) sigma[channel])."""
    g = hostrng.sky_noise_normals(N, seed, dtype).astype(np.float64)
    return (g * sigma[None, None, :]).astype(dtype).astype(np.float64)


def index_map_model(N, seed, mean, std, dtype):
    """k_sky_normal_map with the device generator, before the smoothing: (T)(mean + std double(g))."""
    g = hostrng.sky_index_noise(N, seed, dtype).astype(np.float64)
    return (mean + std * g).astype(dtype).astype(np.float64)


def foreground_model(geo, r, amp, beta, monopole, sigma_pix, N, seed, dtype):
    """The oracle's foreground map fed with the host model of the stream-2 draws."""
    re, im = hostrng.sky_map_noise(N, seed, dtype)
    return so.foreground_amp(geo, r, amp, beta, monopole, sigma_pix=sigma_pix, rng=ReplayNormals(re, im))
