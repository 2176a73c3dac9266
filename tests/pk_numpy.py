"""numpy restatement of CosmoBox.power_spectrum (the definition its kernel implements), in fp64:

    D_a = rfftn(d_a) (unnormalised);  P(k) = (Lx Ly Lz / N^6) Re(conj(D_1) D_2)
    k_a = m_a (2 pi / L_a), m_a the signed FFT index (Nyquist negative); |k| = sqrt((kx kx + ky ky) + kz kz); mu = |kz| / |k|
    modes of the full grid: a half-spectrum cell with 0 < m_z < N/2 counts twice, the planes m_z = 0 and N/2 once; k = 0 excluded
    k bin = np.digitize(|k|, kedges) - 1 (outside [e_0, e_last) dropped); mu bin = np.digitize(mu, linspace(0, 1, Nmu + 1)) - 1,
    mu = 1 in the last bin; per cell: modes, sum |k|, sum mu, sum P, sum P L_l

and a brute-force form over the full np.fft.fftn grid (every mode once) for small N."""
import numpy as np


def signed_index(N):
    i = np.arange(N)
    return np.where(i < N // 2, i, i - N)


def legendre(l, mu):
    m2 = mu * mu
    if l == 0:
        return np.ones_like(mu)
    if l == 2:
        return 1.5 * m2 - 0.5
    if l == 4:
        return ((35. * m2 - 30.) * m2 + 3.) * 0.125
    raise ValueError(l)


def wavenumbers(N, L):
    m = signed_index(N)
    return [m * (2. * np.pi / La) for La in L]


def _bin_cells(K, mu, kedges, Nmu):
    """(cell index, in range) of |k| and mu values by the definition; k = 0 is out of range."""
    nk = kedges.size - 1
    kb = np.digitize(K, kedges) - 1
    mb = np.minimum(np.digitize(mu, np.linspace(0., 1., Nmu + 1)) - 1, Nmu - 1)
    ok = (kb >= 0) & (kb < nk) & (K > 0)
    return kb * Nmu + mb, ok


def _accumulate(cell, ok, w, K, mu, P, nc, lmax, acc):
    c = cell[ok]
    acc[0].append(np.bincount(c, weights=w[ok], minlength=nc))
    acc[1].append(np.bincount(c, weights=(w * K)[ok], minlength=nc))
    acc[2].append(np.bincount(c, weights=(w * mu)[ok], minlength=nc))
    for q, l in enumerate(range(0, lmax + 1, 2)):
        acc[3 + q].append(np.bincount(c, weights=(w * P * legendre(l, mu))[ok], minlength=nc))


def _finish(acc, nk, Nmu, lmax):
    out = [np.sum(np.array(a), axis=0).reshape(nk, Nmu) for a in acc]
    return dict(modes=out[0], sum_k=out[1], sum_mu=out[2], sum_p=out[3],
                sum_pl={l: out[3 + q] for q, l in enumerate(range(0, lmax + 1, 2))})


def power_sums(d1, d2, L, kedges, Nmu=1, lmax=0):
    """Per-cell sums (dict: modes, sum_k, sum_mu, sum_p [nk, Nmu], sum_pl {l: [nk, Nmu]}) from the half spectra."""
    d1 = np.asarray(d1, dtype=np.float64)
    N = d1.shape[0]
    kedges = np.asarray(kedges, dtype=np.float64)
    nk, nc = kedges.size - 1, (kedges.size - 1) * Nmu
    scale = (L[0] * L[1] * L[2]) / float(N) ** 6
    D1 = np.fft.rfftn(d1)
    D2 = D1 if d2 is None else np.fft.rfftn(np.asarray(d2, dtype=np.float64))
    kx, ky, kz = wavenumbers(N, L)
    l = np.arange(N // 2 + 1)
    kzh = kz[l]                                                        # m_z = 0 .. N/2 - 1, then -N/2
    w = np.where((l == 0) | (l == N // 2), 1., 2.)[None, :] * np.ones((N, 1))
    acc = [[] for _ in range(3 + lmax // 2 + 1)]
    for i in range(N):                                                 # one x-plane at a time
        K = np.sqrt((kx[i] * kx[i] + ky[:, None] * ky[:, None]) + kzh[None, :] * kzh[None, :])
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = np.where(K > 0, np.abs(kzh)[None, :] / K, 0.)
        P = scale * (D1[i].real * D2[i].real + D1[i].imag * D2[i].imag)
        cell, ok = _bin_cells(K, mu, kedges, Nmu)
        _accumulate(cell, ok, w, K, mu, P, nc, lmax, acc)
    return _finish(acc, nk, Nmu, lmax)


def power_sums_brute(d1, d2, L, kedges, Nmu=1, lmax=0):
    """The same sums over the full np.fft.fftn grid, every mode counted once (small N)."""
    d1 = np.asarray(d1, dtype=np.float64)
    N = d1.shape[0]
    kedges = np.asarray(kedges, dtype=np.float64)
    nk, nc = kedges.size - 1, (kedges.size - 1) * Nmu
    scale = (L[0] * L[1] * L[2]) / float(N) ** 6
    F1 = np.fft.fftn(d1)
    F2 = F1 if d2 is None else np.fft.fftn(np.asarray(d2, dtype=np.float64))
    kx, ky, kz = wavenumbers(N, L)
    KX, KY, KZ = np.meshgrid(kx, ky, kz, indexing="ij")
    K = np.sqrt((KX * KX + KY * KY) + KZ * KZ)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(K > 0, np.abs(KZ) / K, 0.)
    P = scale * (np.conj(F1) * F2).real
    cell, ok = _bin_cells(K, mu, kedges, Nmu)
    acc = [[] for _ in range(3 + lmax // 2 + 1)]
    _accumulate(cell.ravel(), ok.ravel(), np.ones(K.size), K.ravel(), mu.ravel(), P.ravel(), nc, lmax, acc)
    return _finish(acc, nk, Nmu, lmax)


def power_spectrum(d1, d2, L, kedges, mode="1d", Nmu=5, poles=None, brute=False):
    """What CosmoBox.power_spectrum returns: (k, power, modes) for '1d' (power (len(poles), nk) with poles), or
    (k, mu, power, modes) for '2d'."""
    nmu = Nmu if mode == "2d" else 1
    lmax = 0 if poles is None else max(poles)
    s = (power_sums_brute if brute else power_sums)(d1, d2, L, kedges, nmu, lmax)
    m = s["modes"]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = m == 0
        k = np.where(e, np.nan, s["sum_k"] / m)
        mu = np.where(e, np.nan, s["sum_mu"] / m)
        p = np.where(e, np.nan, s["sum_p"] / m)
        if mode == "2d":
            return k, mu, p, m
        if poles is None:
            return k[:, 0], p[:, 0], m[:, 0]
        pl = np.array([np.where(e[:, 0], np.nan, (2 * l + 1) * s["sum_pl"][l][:, 0] / m[:, 0]) for l in poles])
        return k[:, 0], pl, m[:, 0]
