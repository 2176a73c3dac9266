"""Constructed inputs of the interferometer tests: geometries, channel tables and uv sample sets.  Host only.

A geometry is (N, box_scale) at REDSHIFT; ``HostBox`` carries the attributes ``channel_scales`` reads from a CosmoBox,
computed as CosmoBox computes them, so the tables can be formed without a device (the GPU tests check they are the
box's own, bit for bit).  A case is (name, samples (ns, 2) fp64, mult int32 (ns,) or None)."""
import numpy as np

from fastbox_amd import CosmoBox, default_cosmo
from fastbox_amd.cosmology import Cosmology
from fastbox_amd.interferometer import channel_scales

REDSHIFT = 0.8
GEOMETRIES = {                      # name -> (N, box_scale)
    "n16": (16, 1e3),
    "n18": (18, 1e3),               # N % 4 = 2, not a power of two
    "n30": (30, 1e3),               # coverage kernel: a tail in every wave
    "cuboid": (16, (1e3, 1.5e3, 1.2e3)),
}
RANDOM_NS = (0, 1, 63, 65, 1000)
N_COPIES = 5000


class HostBox(object):
    """The geometry of a CosmoBox (box.py: grid end points, redshift, line frequency) without its engine."""

    freq_array = CosmoBox.freq_array

    def __init__(self, N, box_scale, redshift=REDSHIFT):
        self.cosmo = Cosmology(**default_cosmo) if isinstance(default_cosmo, dict) else default_cosmo
        self.N, self.redshift, self.line_freq = N, redshift, 1420.405752
        scales = box_scale if isinstance(box_scale, tuple) else (box_scale,) * 3
        self.x, self.y, self.z = [np.linspace(-0.5 * s, 0.5 * s, N) for s in scales]
        self.Lx, self.Ly, self.Lz = self.x[-1] - self.x[0], self.y[-1] - self.y[0], self.z[-1] - self.z[0]


def tables(name):
    """(N, sx, sy) of a geometry."""
    N, scale = GEOMETRIES[name]
    sx, sy = channel_scales(HostBox(N, scale))
    return N, sx, sy


def reach(N, s):
    """The baseline component (metres) that lands on cell N/2 in the channel where the table `s` is largest."""
    return 0.5 * N / np.max(s)


def random_set(N, sx, sy, ns, seed):
    """ns baselines with both signs; every channel loses some of them off the grid, the low-frequency end fewer."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-1.6, 1.6, ns) * reach(N, sx), rs.uniform(-1.6, 1.6, ns) * reach(N, sy)], axis=1).reshape(ns, 2)


def everywhere_set(N, sx, sy):
    """For each channel c and each (a, b) in [-N/2, N/2]^2 the sample (a / sx[c], b / sy[c]): every cell of every channel
    is sampled (by that channel's own samples; the others' land where they land)."""
    m = np.arange(-(N // 2), N // 2 + 1, dtype=np.float64)
    a, b = [g.ravel() for g in np.meshgrid(m, m, indexing="ij")]
    return np.concatenate([np.stack([a / sx[c], b / sy[c]], axis=1) for c in range(N)])


def band_edge_set(N, sx, sy):
    """Baselines that fit the grid only where the tables are small: the channels where they are large stay empty."""
    lo, hi = np.min(sx) / np.max(sx), np.min(sy) / np.max(sy)
    f = 1. + 0.5 * (1. / max(lo, hi) - 1.)                # leaves the grid in about half of the band
    rx, ry = reach(N, sx) * f, reach(N, sy) * f
    return np.array([[rx, 0.], [0., ry], [-rx, ry], [rx, ry], [-rx, 0.3 * ry]])


def cases(N, sx, sy):
    """The sample sets every coverage test runs, on the tables of a box."""
    out = [("random%d" % ns, random_set(N, sx, sy, ns, 100 + ns), None) for ns in RANDOM_NS]
    rs = np.random.RandomState(7)
    out.append(("random65-mult", random_set(N, sx, sy, 65, 8), rs.randint(1, 9, 65).astype(np.int32)))
    one = np.array([[0.37 * reach(N, sx), -0.61 * reach(N, sy)]])
    out.append(("copies-expanded", np.repeat(one, N_COPIES, axis=0), None))
    out.append(("copies-collapsed", one, np.array([N_COPIES], dtype=np.int32)))
    out.append(("zero-baseline", np.zeros((1, 2)), np.array([3], dtype=np.int32)))
    out.append(("negative", -np.abs(random_set(N, sx, sy, 40, 9)), None))
    out.append(("everywhere", everywhere_set(N, sx, sy), None))
    out.append(("band-edge", band_edge_set(N, sx, sy), None))
    return out


# ---- hand-made tables, passed straight to the C entry ---------------------------------------------------------------------------
def edge_tables(N):
    """sx = sy = 0.5: an odd component gives an exact half-integer product, 2 a the integer a."""
    return np.full(N, 0.5), np.full(N, 0.5)


def edge_set(N):
    """Ties (odd components: k + 1/2 for every k in reach, both signs), the products exactly on +-N/2 (accepted, folded onto row
    N/2), N/2 + 1/2 (a tie: accepted iff it rounds down, i.e. iff N/2 is even) and the next ones out (rejected)."""
    odd = np.arange(-(N + 3), N + 4, 2, dtype=np.float64)                   # products -(N + 3)/2 .. (N + 3)/2 in steps of 1
    rows = [[v, 0.] for v in odd] + [[0., v] for v in odd] + [[v, -v] for v in odd]
    for v in (float(N), -float(N), N + 2., -(N + 2.)):                      # products +-N/2, +-(N/2 + 1)
        rows += [[v, 0.], [0., v], [v, v], [v, 2.]]
    return np.array(rows)


def upper_empty_tables(N):
    """Tables of 1 cell per metre in the lower half of the band and 10^6 in the upper half, where every non-zero baseline
    leaves the grid."""
    s = np.where(np.arange(N) < N // 2, 1., 1e6)
    return s, s.copy()


def upper_empty_set(N):
    rs = np.random.RandomState(11)
    return np.stack([rs.randint(1, N // 2 + 1, 50) * rs.choice([-1., 1.], 50), rs.randint(1, N // 2 + 1, 50) * 1.], axis=1)


def smooth_cube(N, seed=3):
    """A real cube with structure on every transverse scale and a smooth spectrum along the band, O(1) values."""
    rs = np.random.RandomState(seed)
    return rs.normal(0., 1., (N, N, 1)) * np.linspace(1., 2., N)[None, None, :] + 0.1 * rs.normal(0., 1., (N, N, N)) + 0.5
