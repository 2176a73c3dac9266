"""numpy statement of the COLA particle mesh (CosmoBox.realise_density_cola): numpy FFTs, CIC painting with
np.add.at at fb_paint's nodes, the coefficients of fastbox_amd.cola.  fp64 throughout, unless a stage is given ``dtype``: the
type the device stores Psi1, Psi2, p_res, F, count and delta in.  Every stored value is then rounded to it once, where the
device stores, the transforms run in it (scipy.fft keeps float32) and everything else stays fp64, as on the device."""
import numpy as np
import scipy.fft

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


def stored(x, dtype=np.float64):
    """x rounded once to the stored type, as fp64."""
    return np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)


def _fftn(x, dtype):
    if np.dtype(dtype) == np.float64:
        return np.fft.fftn(x)
    return scipy.fft.fftn(np.asarray(x, dtype=np.float32))             # complex64


def kfield(dk, L, a, b=None, coef=1.0, dtype=np.float64):
    N = dk.shape[0]
    if np.dtype(dtype) == np.float64:
        return np.fft.ifftn(_mult(N, L, a, b, coef) * dk).real
    prod = (_mult(N, L, a, b, coef) * dk.astype(np.complex128)).astype(np.complex64)    # the multiplier is fp64, stored
    return scipy.fft.ifftn(prod).real.astype(np.float64)


def lpt(delta0, L, dtype=np.float64):
    """(Psi1, Psi2), each (3, N, N, N)."""
    dk = _fftn(stored(delta0, dtype), dtype)
    psi1 = np.array([kfield(dk, L, c, dtype=dtype) for c in range(3)])
    xx, yy, zz, xy, xz, yz = [kfield(dk, L, a, b, dtype=dtype)
                              for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    S = ((((xx * yy + xx * zz) + yy * zz) - xy * xy) - xz * xz) - yz * yz
    sk = _fftn(stored(S, dtype), dtype)
    psi2 = np.array([kfield(sk, L, c, coef=-1.0, dtype=dtype) for c in range(3)])
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


def force(pos, N, L, coef, dtype=np.float64):
    """(count, F): count as stored; delta = count - 1 is stored before its transform."""
    count = stored(paint(pos, N, L), dtype)
    dk = _fftn(stored(count - 1., dtype), dtype)
    return count, np.array([kfield(dk, L, c, coef=coef, dtype=dtype) for c in range(3)])


# ---- the transform-free stages, one function per entry point.  psi1, psi2, pres, F: (3, N, N, N) stored values ----------------
def _per_particle(f3):
    return np.asarray(f3, dtype=np.float64).reshape(3, -1).T


def init(psi1, psi2, L, d1, d2):
    """fb_cola_init: positions (N^3, 3) = wrap((q + d1 Psi1) + d2 Psi2)."""
    N = np.asarray(psi1).shape[-1]
    return wrap((lagrangian(N, L) + d1 * _per_particle(psi1)) + d2 * _per_particle(psi2), L)


def kick(F, psi1, psi2, pres, pos, L, coef, drift, dtype=np.float64):
    """fb_cola_kick: (pres (3, N, N, N) as stored, pos)."""
    N = np.asarray(psi1).shape[-1]
    cK, dP1, dP2, Dr, dD1, dD2 = [float(c) for c in coef]
    p1, p2 = _per_particle(psi1), _per_particle(psi2)
    g = readout(np.asarray(F, dtype=np.float64), pos, N, L)
    pn = stored(_per_particle(pres) + ((g * cK - dP1 * p1) - dP2 * p2), dtype)
    if drift:
        pos = wrap(pos + ((pn * Dr + dD1 * p1) + dD2 * p2), L)
    return pn.T.reshape(3, N, N, N), pos


def velocity(psi1, psi2, pres, P1, P2, fac):
    """fb_cola_velocity, all three components: (N^3, 3) fp64."""
    return fac * ((_per_particle(pres) + P1 * _per_particle(psi1)) + P2 * _per_particle(psi2))


def grid_velocity(num, count, dtype=np.float64):
    """fb_cola_grid_velocity: num / count as stored, 0 where count is 0."""
    num, count = np.asarray(num, dtype=np.float64), np.asarray(count, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count != 0., stored(num / count, dtype), 0.)


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
