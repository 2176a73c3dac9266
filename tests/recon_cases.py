"""Constructed inputs for the reconstruction and readout kernels (fb_recon.hip), numpy only: plane waves whose displacement is
known in closed form, a seeded random field, fields whose readout is known by construction, particles on nodes, midpoints and
the seam of the box (tests/particle_cases.py's), and the physical case -- a lattice moved by a Zel'dovich displacement -- on
which reconstruction has to raise the correlation with the linear field.  tests/test_recon_cases_cpu.py holds the numpy
statement (tests/recon_numpy.py) to these cases; tests/test_recon_gpu.py runs them on the device."""
import numpy as np

from tests import particle_cases as pc
from tests import recon_numpy as rn

WINDOWS = rn.WINDOWS


def geometries():
    """[(N, L)]: cubic, cuboid, and N = 18 -- the generic FFT path, N % 4 = 2."""
    return [(16, (32., 32., 32.)), (16, (32., 48., 80.)), (18, (36., 36., 36.))]


WAVES = {"along x": (2, 0, 0), "along z": (0, 0, 3), "oblique": (1, -2, 3)}      # none on a Nyquist plane
PARAMS = dict(R=3., b=1.5, beta=0.4)


def _coords(N, L):
    return [np.arange(N).reshape([N if a == c else 1 for a in range(3)]) * (L[c] / N) for c in range(3)]


def plane_wave(N, L, mode, A=0.25):
    """(delta, k0): delta = A cos(k0.x), k0_a = 2 pi mode_a / L_a."""
    x = _coords(N, L)
    k0 = np.array([2 * np.pi * mode[a] / L[a] for a in range(3)])
    return A * np.cos(k0[0] * x[0] + k0[1] * x[1] + k0[2] * x[2]), k0


def plane_wave_psi(N, L, mode, R, b, beta, A=0.25):
    """The displacement of plane_wave in closed form.  delta(+-k0) = A / 2 and Psi(k) = i k c delta(k) with
    c = exp(-k0^2 R^2 / 2) / (b (k0^2 + beta k0z^2)), so Psi(x) = (i k0 c A / 2) (e^{i k0.x} - e^{-i k0.x}) = -A k0 c sin(k0.x):
    div Psi = -k0^2 c A cos(k0.x), which is -delta_smoothed / b for beta = 0, as the defining equation asks."""
    x = _coords(N, L)
    _, k0 = plane_wave(N, L, mode, A)
    k2 = float(np.dot(k0, k0))
    c = np.exp(-0.5 * k2 * R * R) / (b * (k2 + beta * k0[2] ** 2))
    s = np.sin(k0[0] * x[0] + k0[1] * x[1] + k0[2] * x[2])
    return np.array([-A * k0[a] * c * s for a in range(3)])


def random_field(N, seed=11):
    return 0.2 * np.random.RandomState(seed + N).normal(size=(N, N, N))


def nyquist_mode_spectrum(N, axis):
    """A half spectrum (N, N, N/2 + 1) with the single mode m_axis = -N/2 (1 and 2 on the other two axes; an interior k_z, or
    the stored k_z = N/2 plane for axis 2), and its index."""
    idx = [1, 2, 3]
    idx[axis] = N // 2
    spec = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    spec[tuple(idx)] = 3. - 2.j
    return spec, tuple(idx)


# ---- readout and shift ------------------------------------------------------------------------------------------------------
def readout_fields(N):
    """(3, N, N, N): tests/particle_cases.py field_params -- dyadic values with few bits that differ in every voxel along every
    axis, so that products with the dyadic weights of the constructed positions are exact."""
    return np.array(pc.field_params(N))


def readout_positions(N, L):
    """{name: (n, 3)}: nodes, midpoints and the seam (x = 0, just below L, L, negative inputs that wrap: particle_cases
    paint_positions and below_zero_positions), one particle, 257 particles (a wave tail), none, and a crowd of N^3 / 8 + 3:
    from N^3 / 8 particles on, fb_recon_shift gathers from an interleaved copy of the displacement."""
    seam, _ = pc.paint_positions(N, L)
    below, _ = pc.below_zero_positions(N, L)
    cloud = pc.dyadic_cloud(N, L, 257, 21)
    crowd = np.concatenate([pc.dyadic_cloud(N, L, N ** 3 // 8 + 3 - seam.shape[0], 22), seam])
    return {"seam": np.concatenate([seam, below]), "one": cloud[:1].copy(), "wave tail": cloud,
            "none": np.zeros((0, 3)), "crowd": crowd}


STAGE_DIV = 8                  # FB_RECON_STAGE_DIV of fb_recon.hip


def node_positions(N, L, n=97, seed=4):
    """(pos (n, 3) on mesh nodes, some outside [0, L) by whole boxes; their node indices (n, 3) in [0, N))."""
    rs = np.random.RandomState(seed)
    m = rs.randint(-N, 2 * N, (n, 3))
    return m * (np.asarray(L) / N), np.mod(m, N)


def tsc_node_stencil(field, idx):
    """What TSC reads on a node: (1/8, 3/4, 1/8) along each axis."""
    N = field.shape[0]
    out = np.zeros(idx.shape[0])
    w = (0.125, 0.75, 0.125)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for e in (-1, 0, 1):
                out += (w[a + 1] * w[b + 1]) * w[e + 1] * field[(idx[:, 0] + a) % N, (idx[:, 1] + b) % N, (idx[:, 2] + e) % N]
    return out


def readout_bound(fields, dtype=np.float64):
    """64 * 2^-53 * max|F|: 8 (27 for TSC) products of three rounded weights with a value, with weights that sum to 1.  The
    arithmetic is fp64 on both plans; on an f32 plan the field is rounded to f32 beforehand (``stored``)."""
    return 64. * 2. ** -53 * float(np.max(np.abs(rn.stored(fields, dtype))))


# ---- the physical case ------------------------------------------------------------------------------------------------------
PHYS_N, PHYS_L, PHYS_R, PHYS_SEED = 32, (64., 64., 64.), 3., 5          # cells of 2 Mpc: R = 1.5 cells


def physical_case(f=0.):
    """dict(N, L, R, f, delta_lin, data): a 32^3 lattice moved by the Zel'dovich displacement of a seeded Gaussian field with
    P(k) ~ 1 / k^2 (damped at the Nyquist frequency), scaled to an rms displacement of one cell per axis; with f > 0 the
    particles are in redshift space: x = q + Psi + f Psi_z z^.  delta_lin = -div Psi."""
    N, L = PHYS_N, PHYS_L
    cell = L[0] / N
    rs = np.random.RandomState(PHYS_SEED)
    white = rs.normal(size=(N, N, N))
    _, k = rn.kvec(N, L)
    K = [k[0].reshape(N, 1, 1), k[1].reshape(1, N, 1), k[2][:N // 2 + 1].reshape(1, 1, -1)]
    kk = K[0] ** 2 + K[1] ** 2 + K[2] ** 2
    with np.errstate(divide="ignore"):
        amp = np.where(kk > 0., np.exp(-0.25 * kk * cell * cell) / np.sqrt(kk), 0.)
    dk = np.fft.rfftn(white) * amp
    delta = np.fft.irfftn(dk, s=(N, N, N), axes=(0, 1, 2))
    psi = rn.displacement_k(dk, L, 1e-9, 1., 0.)                       # i k delta / k^2: no smoothing to speak of
    s = cell / np.sqrt(np.mean(psi ** 2))
    psi, delta = psi * s, delta * s
    q = rn.grid_positions(N, L)
    d = psi.reshape(3, -1).T.copy()
    d[:, 2] += f * d[:, 2]
    return dict(N=N, L=L, R=PHYS_R, f=float(f), delta_lin=delta, data=rn.wrap(q + d, L), lattice=q)


def lattice_rms(pos, lattice, L):
    """rms minimum-image distance of pos from its lattice site, in Mpc."""
    L = np.asarray(L)
    d = pos - lattice
    d -= L * np.rint(d / L)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))
