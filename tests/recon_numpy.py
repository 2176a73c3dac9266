"""numpy statement of density-field reconstruction and mesh readout (CosmoBox.reconstruct, .readout,
.uniform_catalogue; fb_recon.hip): np.fft, explicit NGP / CIC / TSC nodes and weights (tests/halos_numpy.py's, which are
fb_paint's), the wrap of tests/cola_numpy.py.  fp64 throughout unless a stage is given ``dtype``, the type the device stores
its fields in: every stored field is then rounded to it once, the transforms run in it (scipy.fft keeps float32) and all
other arithmetic stays fp64, as on the device.

Fourier convention as numpy: f(x) = sum f(k) exp(+i k.x), k_a = 2 pi m_a / L_a, m_a the signed FFT index (N/2 -> -N/2); the
line of sight is z.  tests/test_recon_cases_cpu.py validates this file on its own."""
import numpy as np
import scipy.fft

from fastbox_amd import rng as fb_rng
from tests import halos_numpy as hn
from tests.cola_numpy import stored

WINDOWS = ("ngp", "cic", "tsc")


def kvec(N, L):
    """(m, [k_x, k_y, k_z]) with m the signed index (N/2 -> -N/2) and k_a = (2 pi m) / L_a."""
    m = np.fft.fftfreq(N, 1. / N)
    return m, [(2 * np.pi * m) / La for La in L]


def multipliers(N, L, R, b, beta):
    """The three real multipliers r_a of the half spectrum (N, N, N/2 + 1): Psi_a(k) = i r_a delta(k),
    r_a = k_a exp(-k^2 R^2 / 2) / (b (k^2 + beta k_z^2)); zero at k = 0; r_a zero on the plane m_a = -N/2."""
    m, k = kvec(N, L)
    nz = N // 2 + 1
    K = [k[0].reshape(N, 1, 1), k[1].reshape(1, N, 1), k[2][:nz].reshape(1, 1, nz)]
    M = [m.reshape(N, 1, 1), m.reshape(1, N, 1), m[:nz].reshape(1, 1, nz)]
    kz2 = K[2] * K[2]
    kk = (K[0] * K[0] + K[1] * K[1]) + kz2
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.exp(-0.5 * (kk * (R * R))) / (b * (kk + beta * kz2))
    c[0, 0, 0] = 0.
    return [np.where(M[a] == -(N // 2), 0., K[a] * c) for a in range(3)]


def displacement_k(dk_half, L, R, b, beta, dtype=np.float64):
    """Psi (3, N, N, N) from a half spectrum delta(k) (N, N, N/2 + 1): the 1/N^3 inverse transform of i r_a delta(k)."""
    N = dk_half.shape[0]
    out = []
    for r in multipliers(N, L, R, b, beta):
        prod = 1j * r * dk_half.astype(np.complex128)
        if np.dtype(dtype) == np.float64:
            out.append(np.fft.irfftn(prod, s=(N, N, N), axes=(0, 1, 2)))
        else:
            out.append(scipy.fft.irfftn(prod.astype(np.complex64), s=(N, N, N), axes=(0, 1, 2)).astype(np.float64))
    return np.array(out)


def rfftn(delta, dtype=np.float64):
    if np.dtype(dtype) == np.float64:
        return np.fft.rfftn(np.asarray(delta, dtype=np.float64))
    return scipy.fft.rfftn(np.asarray(delta, dtype=np.float32))                # complex64


def displacement(delta, L, R, b=1., beta=0., dtype=np.float64):
    """Psi (3, N, N, N) of a real density contrast."""
    return displacement_k(rfftn(stored(delta, dtype), dtype), L, R, b, beta, dtype)


def wrap(x, L):
    """x - L floor(x / L) per axis, then + L where negative and - L where >= L (fb_dev.h wrap_pos); x (n, 3)."""
    L = np.asarray(L, dtype=np.float64)
    x = x - L * np.floor(x / L)
    x = np.where(x < 0., x + L, x)
    return np.where(x >= L, x - L, x)


def readout(fields, pos, L, window="cic"):
    """(n, k): the k fields (k, N, N, N) read at pos (n, 3) through the window: sum over its nodes, x outermost, of
    ((w_x w_y) w_z) F[node].  fb_paint's nodes and weights (tests/halos_numpy.py _axis)."""
    fields = np.asarray(fields, dtype=np.float64)
    N = fields.shape[1]
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ax = [hn._axis(pos[:, a] * (N / L[a]), window, N) for a in range(3)]
    g = np.zeros((pos.shape[0], fields.shape[0]))
    for m0, w0 in ax[0]:
        for m1, w1 in ax[1]:
            wab = w0 * w1
            for m2, w2 in ax[2]:
                wt = wab * w2
                i = tuple(np.mod(m, N).astype(np.int64) for m in (m0, m1, m2))
                for c in range(fields.shape[0]):
                    g[:, c] += wt * fields[c][i]
    return g


def shift(psi, pos, L, window="cic", scale=1., scale_z=0.):
    """wrap(x - scale Psi(x) - scale_z Psi_z(x) z^): along z, x_z - (scale Psi_z + scale_z Psi_z)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    g = readout(psi, pos, L, window)
    d = scale * g
    d[:, 2] = scale * g[:, 2] + scale_z * g[:, 2]
    return wrap(pos - d, L)


def grid_positions(N, L):
    """(N^3, 3): one particle on each mesh node, C order (randoms='grid')."""
    g = np.meshgrid(*[np.arange(N, dtype=np.float64) * (La / N) for La in L], indexing="ij")
    return np.stack([c.reshape(-1) for c in g], axis=1)


def density_contrast(pos, N, L, window="cic", dtype=np.float64):
    """delta = n / nbar - 1 of a catalogue: the painted mesh (stored) times N^3 / n, minus 1 (stored)."""
    mesh = stored(hn.paint(pos, N, L, window), dtype)
    return stored(mesh * (float(N) ** 3 / pos.shape[0]) - 1., dtype)


def reconstruct(data, randoms, N, L, R, b=1., f=0., convention="sym", window="cic", delta=None, dtype=np.float64):
    """dict(delta_rec, data, randoms, psi): the whole pipeline.  ``randoms``: (n, 3) positions."""
    if convention not in ("sym", "iso"):
        raise ValueError(convention)
    data = np.asarray(data, dtype=np.float64).reshape(-1, 3)
    if delta is None:
        delta = density_contrast(data, N, L, window, dtype)
    psi = stored(displacement(delta, L, R, b, f / b, dtype), dtype)
    sd = shift(psi, data, L, window, 1., f)
    sr = shift(psi, randoms, L, window, 1., f if convention == "sym" else 0.)
    D = stored(hn.paint(sd, N, L, window), dtype)
    S = stored(hn.paint(sr, N, L, window), dtype)
    n3 = float(N) ** 3
    rec = stored(D * (n3 / sd.shape[0]) - S * (n3 / sr.shape[0]), dtype)
    return dict(delta_rec=rec, data=sd, randoms=sr, psi=psi)


def uniform_positions(n, L, seed, realisation=0):
    return fb_rng.recon_uniforms(n, L, seed, realisation)


def kbins(N, L, nbins=8):
    """nbins equal bins of |k| from 0 (exclusive) to the Nyquist frequency of the coarsest axis."""
    return np.linspace(0., np.pi * N / max(L), nbins + 1)


def cross_correlation(a, b, L, nbins=8):
    """r(k) = sum Re(a b*) / sqrt(sum |a|^2 sum |b|^2) over the modes of each |k| bin of ``kbins`` (upper edge inclusive)."""
    N = a.shape[0]
    ak, bk = np.fft.fftn(a), np.fft.fftn(b)
    _, k = kvec(N, L)
    kk = np.sqrt(k[0].reshape(N, 1, 1) ** 2 + k[1].reshape(1, N, 1) ** 2 + k[2].reshape(1, 1, N) ** 2)
    edges = kbins(N, L, nbins)
    idx = np.searchsorted(edges, kk.reshape(-1), side="left") - 1                # (e_j, e_j+1]
    ok = (idx >= 0) & (idx < nbins)
    def binned(v):
        return np.bincount(idx[ok], weights=v.reshape(-1)[ok], minlength=nbins)
    pab, paa, pbb = binned((ak * np.conj(bk)).real), binned(np.abs(ak) ** 2), binned(np.abs(bk) ** 2)
    return pab / np.sqrt(paa * pbb)
