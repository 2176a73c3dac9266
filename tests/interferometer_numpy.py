"""The statement of the interferometer feature in numpy: what fb_uv_coverage, fb_uv_channel_sums, fb_uv_weight and
Interferometer.observe / psf / noise compute.  Host only; shared by the CPU and the GPU tests.

Cubes are (N, N, N) with the frequency channel last; transforms are np.fft's over axes (0, 1)."""
import numpy as np

NATURAL, UNIFORM, SQRT = 0, 1, 2
MODES = {"natural": NATURAL, "uniform": UNIFORM}


def coverage(N, samples, mult, sx, sy, counts=None):
    """S int32 (N, N, N).  Sample s in channel c, all fp64: a = rint(bx sx[c]), b = rint(by sy[c]); accepted iff |a| <= N/2
    and |b| <= N/2; then m goes to S[a mod N][b mod N][c] and to S[-a mod N][-b mod N][c].  mult None: all 1.  counts: the cube
    to accumulate into (not modified)."""
    S = np.zeros((N, N, N), dtype=np.int32) if counts is None else np.array(counts, dtype=np.int32)
    samples = np.asarray(samples, dtype=np.float64).reshape(-1, 2)
    if samples.shape[0] == 0:
        return S
    m = np.ones(samples.shape[0], dtype=np.int32) if mult is None else np.asarray(mult, dtype=np.int32)
    with np.errstate(all="ignore"):
        a = np.rint(samples[:, 0, None] * np.asarray(sx, dtype=np.float64)[None, :])
        b = np.rint(samples[:, 1, None] * np.asarray(sy, dtype=np.float64)[None, :])
        ok = (np.abs(a) <= N // 2) & (np.abs(b) <= N // 2)
    s_at, c_at = np.nonzero(ok)
    ia, ib = a[ok].astype(np.int64), b[ok].astype(np.int64)
    np.add.at(S, (ia % N, ib % N, c_at), m[s_at])
    np.add.at(S, ((-ia) % N, (-ib) % N, c_at), m[s_at])
    return S


def accepted_multiplicity(N, samples, mult, sx, sy):
    """Per channel, the sum of the multiplicities of the accepted samples (int64 (N,))."""
    samples = np.asarray(samples, dtype=np.float64).reshape(-1, 2)
    m = np.ones(samples.shape[0], dtype=np.int64) if mult is None else np.asarray(mult, dtype=np.int64)
    with np.errstate(all="ignore"):
        a = np.rint(samples[:, 0, None] * sx[None, :])
        b = np.rint(samples[:, 1, None] * sy[None, :])
        ok = (np.abs(a) <= N // 2) & (np.abs(b) <= N // 2)
    return (ok * m[:, None]).sum(axis=0).astype(np.int64)


def channel_sums(S):
    """(tot, ncell): int64 (N,) each."""
    return S.sum(axis=(0, 1), dtype=np.int64), (S > 0).sum(axis=(0, 1), dtype=np.int64)


def factor(S, mode, scale):
    """f(S) scale[c] in fp64: f = S, [S > 0] or sqrt(S)."""
    S = np.asarray(S)
    f = S.astype(np.float64) if mode == NATURAL else (S > 0).astype(np.float64) if mode == UNIFORM else np.sqrt(S.astype(np.float64))
    return f * np.asarray(scale, dtype=np.float64)[None, None, :]


def weight(spec, S, mode, scale):
    """fb_uv_weight on a complex64 / complex128 cube: each component times the fp64 factor, in fp64, rounded once to the
    cube's precision."""
    spec = np.asarray(spec)
    rdt = np.float32 if spec.dtype == np.complex64 else np.float64
    fac = factor(S, mode, scale)
    out = np.empty(spec.shape, dtype=spec.dtype)
    out.real = (spec.real.astype(np.float64) * fac).astype(rdt)
    out.imag = (spec.imag.astype(np.float64) * fac).astype(rdt)
    return out


def normaliser(S, weighting):
    """N^2 / w[c], 0 where w = 0; w = tot (natural) or ncell (uniform)."""
    tot, ncell = channel_sums(S)
    w = (tot if weighting == "natural" else ncell).astype(np.float64)
    out = np.zeros(w.size)
    np.divide(float(S.shape[0]) ** 2, w, out=out, where=w > 0)
    return out


def apply(cube, S, mode, scale):
    """ifft2(fft2(cube) f(S) scale[c]) per channel, complex128."""
    spec = np.fft.fft2(np.asarray(cube, dtype=np.float64), axes=(0, 1))
    return np.fft.ifft2(spec * factor(S, mode, scale), axes=(0, 1))


def observe(cube, S, weighting="natural", beam=None):
    """D[:, :, c] = ifft2(fft2(A T)[:, :, c] f(S[:, :, c])) N^2 / w[c] (complex128: the imaginary part is rounding)."""
    field = np.asarray(cube, dtype=np.float64)
    if beam is not None:
        field = np.asarray(beam, dtype=np.float64) * field
    return apply(field, S, MODES[weighting], normaliser(S, weighting))


def impulse(N, at=(0, 0)):
    cube = np.zeros((N, N, N))
    cube[at[0], at[1], :] = 1.
    return cube


def psf(S, weighting="natural"):
    return observe(impulse(S.shape[0]), S, weighting)


def noise_scale(S, sigma):
    """N sigma_c / tot[c], 0 in an empty channel."""
    N = S.shape[0]
    tot = channel_sums(S)[0].astype(np.float64)
    out = np.zeros(N)
    np.divide(float(N) * np.broadcast_to(np.asarray(sigma, dtype=np.float64), (N,)), tot, out=out, where=tot > 0)
    return out


def noise(g, S, sigma):
    """n[:, :, c] = N sigma_c ifft2(sqrt(S) fft2(g)) / tot[c] for the unit white real cube g (complex128)."""
    return apply(g, S, SQRT, noise_scale(S, sigma))
