"""numpy restatement of CosmoBox.cylindrical_power_spectrum and CosmoBox.angular_power_spectrum (the definitions their kernels
implement), in fp64, independent of fastbox_amd.hostgeom:

    k_a = m_a (2 pi / L_a), m_a the signed FFT index (Nyquist negative); k_perp = sqrt(kx kx + ky ky); k_par = |kz|
    bins: np.digitize(x, edges) - 1, values outside [e_0, e_last) dropped

    cylindrical: D_a = rfftn(d_a) (unnormalised); P = (Lx Ly Lz / N^6) Re(conj(D_1) D_2); modes of the full grid (a half-spectrum
    cell with 0 < m_z < N/2 counts twice, the planes m_z = 0 and N/2 once), k = 0 excluded; per cell modes, sum k_perp,
    sum k_par, sum P.

    angular: a_a = np.fft.fftn(d_a, axes=(0, 1)) (unnormalised), every m_perp of the N x N plane but 0;
    C_b(nu, nu') = (Lx Ly / N^4) (1 / modes_b) sum_{m_perp in b} Re(a_1(m_perp, nu) conj(a_2(m_perp, nu')))."""
import numpy as np


def signed_index(N):
    i = np.arange(N)
    return np.where(i < N // 2, i, i - N)


def wavenumbers(N, L):
    m = signed_index(N)
    return [m * (2. * np.pi / La) for La in L]


def kperp_plane(N, L):
    kx, ky, _ = wavenumbers(N, L)
    return np.sqrt(kx[:, None] * kx[:, None] + ky[None, :] * ky[None, :])


def _digitize(x, edges):
    b = np.digitize(x, edges) - 1
    return b, (b >= 0) & (b < edges.size - 1)


def cyl_sums(d1, d2, L, perp_edges, par_edges):
    """Per-cell sums (dict: modes, sum_kperp, sum_kpar, sum_p, each [nperp, npar]) from the half spectra."""
    d1 = np.asarray(d1, dtype=np.float64)
    N = d1.shape[0]
    pe, qe = np.asarray(perp_edges, dtype=np.float64), np.asarray(par_edges, dtype=np.float64)
    nperp, npar = pe.size - 1, qe.size - 1
    nc = nperp * npar
    scale = (L[0] * L[1] * L[2]) / float(N) ** 6
    D1 = np.fft.rfftn(d1)
    D2 = D1 if d2 is None else np.fft.rfftn(np.asarray(d2, dtype=np.float64))
    kz = wavenumbers(N, L)[2]
    l = np.arange(N // 2 + 1)
    kpar = np.abs(kz[l])                                               # m_z = 0 .. N/2 - 1, then -N/2
    w = np.where((l == 0) | (l == N // 2), 1., 2.)[None, :] * np.ones((N, 1))
    KP = kperp_plane(N, L)
    acc = [[] for _ in range(4)]
    for i in range(N):                                                 # one x-plane at a time
        kp = KP[i][:, None] * np.ones((1, l.size))
        kq = np.ones((N, 1)) * kpar[None, :]
        P = scale * (D1[i].real * D2[i].real + D1[i].imag * D2[i].imag)
        b, okb = _digitize(kp, pe)
        c, okc = _digitize(kq, qe)
        ok = okb & okc & ((kp > 0) | (kq > 0))                         # k = 0 excluded
        cell = (b * npar + c)[ok]
        for q, v in enumerate((w, w * kp, w * kq, w * P)):
            acc[q].append(np.bincount(cell, weights=v[ok], minlength=nc))
    out = [np.sum(np.array(a), axis=0).reshape(nperp, npar) for a in acc]
    return dict(modes=out[0], sum_kperp=out[1], sum_kpar=out[2], sum_p=out[3])


def cyl_sums_brute(d1, d2, L, perp_edges, par_edges):
    """The same sums over the full np.fft.fftn grid with np.add.at, every mode counted once (small N)."""
    d1 = np.asarray(d1, dtype=np.float64)
    N = d1.shape[0]
    pe, qe = np.asarray(perp_edges, dtype=np.float64), np.asarray(par_edges, dtype=np.float64)
    nperp, npar = pe.size - 1, qe.size - 1
    scale = (L[0] * L[1] * L[2]) / float(N) ** 6
    F1 = np.fft.fftn(d1)
    F2 = F1 if d2 is None else np.fft.fftn(np.asarray(d2, dtype=np.float64))
    kz = wavenumbers(N, L)[2]
    kp = kperp_plane(N, L)[:, :, None] * np.ones((1, 1, N))
    kq = np.ones((N, N, 1)) * np.abs(kz)[None, None, :]
    P = scale * (np.conj(F1) * F2).real
    b, okb = _digitize(kp, pe)
    c, okc = _digitize(kq, qe)
    ok = okb & okc & ((kp > 0) | (kq > 0))
    out = np.zeros((4, nperp, npar))
    for q, v in enumerate((np.ones_like(kp), kp, kq, P)):
        np.add.at(out[q], (b[ok], c[ok]), v[ok])
    return dict(modes=out[0], sum_kperp=out[1], sum_kpar=out[2], sum_p=out[3])


def cylindrical_power_spectrum(d1, d2, L, perp_edges, par_edges, brute=False):
    """What CosmoBox.cylindrical_power_spectrum returns: (kperp, kpar, power, modes), each (nperp, npar)."""
    s = (cyl_sums_brute if brute else cyl_sums)(d1, d2, L, perp_edges, par_edges)
    m = s["modes"]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = m == 0
        return (np.where(e, np.nan, s["sum_kperp"] / m), np.where(e, np.nan, s["sum_kpar"] / m),
                np.where(e, np.nan, s["sum_p"] / m), m)


def angular_power_spectrum(d1, d2, L, perp_edges):
    """What CosmoBox.angular_power_spectrum returns: (kperp (nb,), cl (nb, N, N), modes (nb,) int64)."""
    d1 = np.asarray(d1, dtype=np.float64)
    N = d1.shape[0]
    pe = np.asarray(perp_edges, dtype=np.float64)
    nb = pe.size - 1
    a1 = np.fft.fftn(d1, axes=(0, 1)).reshape(N * N, N)
    a2 = a1 if d2 is None else np.fft.fftn(np.asarray(d2, dtype=np.float64), axes=(0, 1)).reshape(N * N, N)
    kp = kperp_plane(N, L).ravel()
    b, ok = _digitize(kp, pe)
    ok[0] = False                                                      # m_perp = 0
    kperp, cl, modes = np.full(nb, np.nan), np.full((nb, N, N), np.nan), np.zeros(nb, dtype=np.int64)
    for q in range(nb):
        sel = ok & (b == q)
        modes[q] = np.count_nonzero(sel)
        if modes[q] == 0:
            continue
        kperp[q] = np.sum(kp[sel]) / modes[q]
        x, y = a1[sel], a2[sel]
        cl[q] = (L[0] * L[1] / float(N) ** 4) * (x.real.T @ y.real + x.imag.T @ y.imag) / modes[q]
    return kperp, cl, modes


def collapse(cl):
    """(nb, N): the mean of cl[b, nu, nu + D] over the N - D pairs, by loops."""
    nb, N, _ = cl.shape
    out = np.zeros((nb, N))
    for b in range(nb):
        for D in range(N):
            out[b, D] = sum(cl[b, nu, nu + D] for nu in range(N - D)) / (N - D)
    return out


def power_from_maps(cl, Lz):
    """The identity tying the two estimators: P(b, m) = (Lz / N^2) sum_{nu, nu'} C_b(nu, nu') cos(2 pi m (nu - nu') / N),
    m = 0 .. N/2; (nb, N/2 + 1)."""
    nb, N, _ = cl.shape
    nu = np.arange(N)
    out = np.zeros((nb, N // 2 + 1))
    for m in range(N // 2 + 1):
        out[:, m] = (Lz / float(N) ** 2) * np.sum(cl * np.cos(2. * np.pi * m * (nu[:, None] - nu[None, :]) / N)[None], axis=(1, 2))
    return out
