"""numpy statement of the COLA particle mesh (CosmoBox.realise_density_cola): numpy FFTs, CIC painting with
np.add.at at fb_paint's nodes, the coefficients of fastbox_amd.cola.  fp64 throughout."""
import numpy as np

from fastbox_amd import cola


def kvec(N, L):
    m = np.fft.fftfreq(N, 1. / N)                       # signed index, N/2 -> -N/2
    k = 2 * np.pi * m / L
    return m, k


def _mult(N, L, a, b=None, coef=1.0):
    """The multiplier of fb_cola_lpt / fb_cola_force on the full (N, N, N) grid."""
    m, k = kvec(N, L)
    sh = [(N, 1, 1), (1, N, 1), (1, 1, N)]
    K = [k.reshape(s) for s in sh]
    M = [m.reshape(s) for s in sh]
    kk = (K[0] * K[0] + K[1] * K[1]) + K[2] * K[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        if b is None:
            r = (coef * K[a]) / kk * np.ones((N, N, N))
            r = np.where(M[a] == -N // 2, 0., r)
            r = 1j * r
        else:
            r = (coef * (K[a] * K[b])) / kk * np.ones((N, N, N))
            if a != b:
                r = np.where((M[a] == -N // 2) | (M[b] == -N // 2), 0., r)
    r[0, 0, 0] = 0.
    return r


def kfield(dk, L, a, b=None, coef=1.0):
    N = dk.shape[0]
    return np.fft.ifftn(_mult(N, L, a, b, coef) * dk).real


def lpt(delta0, L):
    """(Psi1, Psi2), each (3, N, N, N)."""
    dk = np.fft.fftn(delta0)
    psi1 = np.array([kfield(dk, L, c) for c in range(3)])
    xx, yy, zz, xy, xz, yz = [kfield(dk, L, a, b) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    S = ((((xx * yy + xx * zz) + yy * zz) - xy * xy) - xz * xz) - yz * yz
    sk = np.fft.fftn(S)
    psi2 = np.array([kfield(sk, L, c, coef=-1.0) for c in range(3)])
    return psi1, psi2


def wrap(x, L):
    x = x - L * np.floor(x / L)
    x = np.where(x < 0., x + L, x)
    return np.where(x >= L, x - L, x)


def lagrangian(N, L):
    """(N^3, 3) nodes m L / N in C order."""
    i = np.arange(N, dtype=np.float64) * (L / N)
    g = np.meshgrid(i, i, i, indexing="ij")
    return np.stack([c.reshape(-1) for c in g], axis=1)


def cic_nodes(pos, N, L):
    """Nodes (n, 8) and weights (n, 8) of fb_paint's CIC."""
    u = pos * (N / L)
    f0 = np.floor(u)
    f = u - f0
    m0 = np.mod(f0.astype(np.int64), N)
    m1 = np.mod(f0.astype(np.int64) + 1, N)
    ms, ws = (m0, m1), (1. - f, f)
    nodes, wts = [], []
    for a in range(2):
        for b in range(2):
            for e in range(2):
                nodes.append((ms[a][:, 0] * N + ms[b][:, 1]) * N + ms[e][:, 2])
                wts.append((ws[a][:, 0] * ws[b][:, 1]) * ws[e][:, 2])
    return np.stack(nodes, 1), np.stack(wts, 1)


def paint(pos, N, L, w=None):
    nodes, wts = cic_nodes(pos, N, L)
    if w is not None:
        wts = wts * w[:, None]
    out = np.zeros(N ** 3)
    np.add.at(out, nodes.reshape(-1), wts.reshape(-1))
    return out.reshape(N, N, N)


def readout(field3, pos, N, L):
    nodes, wts = cic_nodes(pos, N, L)
    return np.stack([np.sum(wts * f.reshape(-1)[nodes], axis=1) for f in field3], axis=1)


def force(pos, N, L, coef):
    count = paint(pos, N, L)
    dk = np.fft.fftn(count - 1.)
    return count, np.array([kfield(dk, L, c, coef=coef) for c in range(3)])


def run(delta0, L, cosmo, redshift, redshift_init, n_steps, h=None):
    """Returns dict: pos (N^3, 3), pres, psi1, psi2 (N^3, 3), delta (N, N, N), vel (N^3, 3) km/s, grid_vel (3, N, N, N)."""
    N = delta0.shape[0]
    g = cola.Growth(cosmo)
    tab = cola.launch_table(g, redshift, redshift_init, n_steps)
    psi1, psi2 = lpt(delta0, L)
    p1 = psi1.reshape(3, -1).T
    p2 = psi2.reshape(3, -1).T
    pos = wrap((lagrangian(N, L) + tab[0] * p1) + tab[1] * p2, L)
    pres = np.zeros_like(pos)
    if n_steps == 0:
        count = paint(pos, N, L)
    for j in range(n_steps + 1 if n_steps else 0):
        count, F = force(pos, N, L, tab[2])
        cK, dP1, dP2, Dr, dD1, dD2 = tab[3 + 6 * j: 9 + 6 * j]
        Fp = readout(F, pos, N, L)
        pres = pres + ((Fp * cK - dP1 * p1) - dP2 * p2)
        if j < n_steps:
            pos = wrap(pos + ((pres * Dr + dD1 * p1) + dD2 * p2), L)
    h = cosmo['h'] if h is None else h
    P1, P2, fac = cola.velocity_coefficients(g, redshift, h)
    vel = fac * ((pres + P1 * p1) + P2 * p2)
    with np.errstate(divide="ignore", invalid="ignore"):
        gv = np.array([np.where(count != 0., paint(pos, N, L, vel[:, c]) / count, 0.) for c in range(3)])
    return dict(pos=pos, pres=pres, psi1=p1, psi2=p2, delta=count - 1., vel=vel, grid_vel=gv)
