"""
Host-side geometry of a CosmoBox that needs no GPU: grid, |k| shells, bin edges and the
per-bin shell thresholds handed to the device.  Every expression follows the reference's
numpy arithmetic (fastbox/box.py lines cited) so that |k| and np.digitize agree bit for bit.
Shared by ``CosmoBox`` (single GPU) and ``SlabBox`` (one box over several GPUs).
"""
import numpy as np


def grid(box_scale, nsamp):
    """x, y, z (linspace incl. both end points), side lengths, boxfactor, kmin, kmax
    (box.py:76-101)."""
    if isinstance(box_scale, tuple):
        assert len(box_scale) == 3, "Must specify scale of x, y, z dimensions"
        x, y, z = [np.linspace(-0.5 * s, 0.5 * s, nsamp) for s in box_scale]
    else:
        x = y = z = np.linspace(-0.5 * box_scale, 0.5 * box_scale, nsamp)
    L = (x[-1] - x[0], y[-1] - y[0], z[-1] - z[0])
    boxfactor = (nsamp ** 6.) / (L[0] * L[1] * L[2])
    kmin = 2. * np.pi / np.max(L)
    kmax = 2. * np.pi * np.sqrt(3.) * nsamp / np.min(L)
    return dict(N=nsamp, x=x, y=y, z=z, L=L, boxfactor=boxfactor, kmin=kmin, kmax=kmax,
                cubic=(L[0] == L[1] == L[2]))


def mode_numbers(N):
    """The integer mode number the reference's k grid carries at every index (box.py:119-123):

        NN = (N * fftfreq(N, 1.)).astype("i");  for i in NN: Kx[i, :, :] = i

    -- `i` is index AND value.  For a power of two the product is exact and this is fftfreq's numbering.  For other N the
    product can round just below an integer (24 * (7/24) = 6.999...), the cast truncates, NN then holds 6 twice and 7 never,
    and Kx[7] keeps the 0 it was initialised with.  Reproduced as it is: same inputs, same results as the reference."""
    nn = (N * np.fft.fftfreq(N, 1.)).astype("i")
    m = np.zeros(N, dtype=np.float64)
    for i in nn:
        m[i] = i
    return m


def axis_tables(N, L):
    """(m/L)**2 per axis [3N], m*(2 pi/L) per axis [3N], 2 pi m / Lz [N]
    (box.py:125-127, 254-256, 375)."""
    m = mode_numbers(N)
    axis2 = np.concatenate([(m / l) ** 2. for l in L])
    ksc = np.concatenate([m * (2. * np.pi / l) for l in L])
    kpar = 2. * np.pi * m / L[2]
    return axis2, ksc, kpar


def shell_wavenumbers(N, Lside):
    """|k| of every integer shell n^2 = i^2 + j^2 + l^2 of a cubic box."""
    n2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    return 2. * np.pi * np.sqrt(n2) / Lside


def shell_amplitude(N, Lside, boxfactor, pk_fn):
    """sqrt(nan_to_num(P(k)) * boxfactor) per shell (box.py:161-171)."""
    with np.errstate(all="ignore"):
        pk = np.nan_to_num(np.asarray(pk_fn(shell_wavenumbers(N, Lside)), dtype=np.float64))
        return np.sqrt(pk * boxfactor)


def shell_multiplicity(N):
    """Number of modes (i, j, l) of the full (N, N, N) grid on every integer shell n^2 = i^2 + j^2 + l^2."""
    m2 = (mode_numbers(N) ** 2).astype(np.int64)
    h2 = np.bincount((m2[:, None] + m2[None, :]).ravel())            # pairs (i, j)
    out = np.zeros(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    vals, cnt = np.unique(m2, return_counts=True)
    for v, c in zip(vals, cnt):
        out[v:v + h2.size] += c * h2
    return out


def field_variance_cubic(N, amp_shells):
    """Variance of the realised field whose modes have E|delta_k|^2 = amp^2: sum_k amp_k^2 / N^6 (Parseval)."""
    a = np.asarray(amp_shells, dtype=np.float64)
    return float(np.sum(shell_multiplicity(N)[:a.size] * a * a) / float(N) ** 6)


def field_variance_sym(N, amp_sym):
    """The same from the (|m_x|, |m_y|, |m_z|) table of a box of any shape (N/2+1 entries per axis)."""
    w = np.full(N // 2 + 1, 2.0)
    w[0] = w[-1] = 1.0
    a = np.asarray(amp_sym, dtype=np.float64)
    return float(np.einsum("i,j,k,ijk->", w, w, w, a * a) / float(N) ** 6)


LN_SUM_MAX = 21.0        # ln of the largest sum of shifted exponentials a single-precision plan can carry: the k = 0
                         # mode of the transform IS that sum and its |.|^4 must stay below 2^128 (e^88.7)


def lognormal_shift(sigma2, nvox):
    """Shift c of the fused log-normal transform, which forms exp(delta - c): the estimate exp(d)/<exp(d)> - 1
    (box.py:457-460) and its P(k) do not depend on c, but on a single-precision plan the sums only stay in range
    for the right c.  Chosen from where S = sum exp(delta) of nvox Gaussian values of variance sigma2 will lie:

      sigma <= a = sqrt(2 ln nvox):  the sum is the sample mean's,  ln S = ln nvox + sigma^2/2  ->  S e^-c = e^7
      sigma >  a                  :  the sum is its few largest terms, ln S ~ max delta, a Gumbel variable of
                                     location mu = sigma (a - (ln ln nvox + ln 4 pi) / (2 a)) and scale sigma / a
                                     ->  the largest term lands at e^-6 (27 e-folds of head room above, since the
                                     upper tail of the maximum is the wide one; 14 below before anything that
                                     matters flushes to zero)

    (sigma^2/2, round 2's choice, is the first line without the ln nvox; past sigma ~ 13 it puts EVERY term below
    the single-precision range: 2048^3 at 2 Mpc/voxel has sigma = 21 and max delta - sigma^2/2 = -94.)
    A realisation that falls outside the range anyway is detected by its non-finite sums and repeated with the
    exact shift, `lognormal_shift_exact`."""
    sigma2 = max(float(sigma2), 0.0)
    if sigma2 == 0.0 or nvox < 2:
        return 0.0
    sigma, ln_n = np.sqrt(sigma2), np.log(float(nvox))
    a = np.sqrt(2. * ln_n)
    if sigma <= a:
        return float(ln_n + 0.5 * sigma2 - 7.0)
    mu = sigma * (a - (np.log(ln_n) + np.log(4. * np.pi)) / (2. * a))
    return float(mu + 6.0)


def lognormal_shift_exact(dmax, nvox):
    """The shift for a field whose maximum is known: every term is <= e^-m with m = max(0, ln nvox - LN_SUM_MAX),
    so the sum lies in [e^-m, e^LN_SUM_MAX] whatever the field looks like."""
    return float(dmax) + max(0.0, np.log(float(nvox)) - LN_SUM_MAX)


def lognormal_sums_in_range(cnt, s1, s2, esum):
    """Did the shifted exponentials of a fused log-normal P(k) stay inside the plan's floating-point range?
    Overflow shows as non-finite sums (or a sum of exponentials that is not a positive number); underflow as a
    non-empty bin whose sum of squares has lost terms, i.e. lies below (sum)^2 / n, which no set of real numbers
    does.  Bin 0 is the reference's discarded one (box.py:761-764) and is not looked at."""
    c = np.asarray(cnt)[1:]
    ok = c > 0
    a, b = np.asarray(s1)[1:][ok], np.asarray(s2)[1:][ok]
    if not (np.isfinite(esum) and esum > 0. and np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return False
    # (a bin with exactly zero power -- a constant field: exp(d)/mean - 1 = 0, the reference returns P = 0 -- is in range: with a
    # finite, positive sum of exponentials underflow cannot produce it)
    zero = (a == 0.) & (b == 0.)
    return bool(np.all((a > 0.) | zero) and np.all(b * c[ok] >= a * a * (1. - 1e-3)))


def lognormal_sums_in_range_many(cnt, s1, s2, esum):
    """`lognormal_sums_in_range` for many records at once: s1, s2 (records, nbins), esum (records,) -> bool per record."""
    c = np.asarray(cnt)[1:]
    ok = c > 0
    a, b = np.asarray(s1)[:, 1:][:, ok], np.asarray(s2)[:, 1:][:, ok]
    with np.errstate(all="ignore"):
        fin = np.isfinite(esum) & (esum > 0.) & np.all(np.isfinite(a), axis=1) & np.all(np.isfinite(b), axis=1)
        zero = (a == 0.) & (b == 0.)
        return fin & np.all((a > 0.) | zero, axis=1) & np.all(b * c[ok] >= a * a * (1. - 1e-3), axis=1)


def lognormal_rescale(s1, s2, mean):
    """Bin sums of the transform of exp(d - shift), brought to those of exp(d)/<exp(d)> - 1: s1 / mean^2, s2 / mean^4, with
    mean = sum(exp(d - shift)) / voxels (scalar, or one per record for (records, nbins) sums).  The powers are formed by
    multiplications -- exactly rounded on every platform, for a Python float as for a numpy array, which `mean ** 4` is
    not (numpy's vectorised pow and libm's differ in the last bit on some hosts): one record finished alone and the same
    record finished in a batch give the same numbers."""
    m2 = mean * mean
    m4 = m2 * m2
    if np.ndim(mean):
        m2, m4 = m2[:, None], m4[:, None]
    return s1 / m2, s2 / m4


def finish_bins_many(cnt, s1, s2, boxfactor, eps=0.):
    """`finish_bins` for many records at once (s1, s2: (records, nbins)); the same expressions, element for element."""
    with np.errstate(all="ignore"):
        vals = s1 / (cnt * boxfactor)
        var = (s2 - s1 * s1 / cnt) / cnt
        if eps:
            var = np.where((cnt <= 2) & (var <= 4. * eps * (s1 / cnt) ** 2), 0., var)
        stddev = np.sqrt(np.maximum(var, 0.)) / boxfactor / np.sqrt(cnt)
    return vals[:, 1:], stddev[:, 1:]


def bin_edges(g, nbins=20, kbins=None):
    """Edges and the centres of bins 1..nbins-1 (box.py:745-751)."""
    if kbins is not None:
        bins = np.asarray(kbins, dtype=np.float64)
    else:
        bins = np.logspace(np.log10(g["kmin"]), np.log10(g["kmax"]), nbins)
    _b = [0.0] + list(bins)
    cent = [0.5 * (_b[j + 1] + _b[j]) for j in range(bins.size)]
    return bins, np.array(cent[1:])


def shell_thresholds(N, Lside, bins):
    """np.digitize(k, bins) as a step function of the integer shell (cubic boxes): thr[b] = first
    n^2 whose bin index exceeds b.  Shells whose |k| lies within rounding of an edge cannot be
    decided from n^2 alone (the reference's per-mode |k| differs in the last bits between
    decompositions of the same n^2) and are returned in `amb` for the exact on-device path."""
    if not np.all(np.diff(bins) >= 0):
        return None, ()
    k = shell_wavenumbers(N, Lside)
    eps = 64 * np.finfo(np.float64).eps
    lo = np.digitize(k * (1. - eps), bins)
    hi = np.digitize(k * (1. + eps), bins)
    amb = np.nonzero(lo != hi)[0]
    if amb.size > 8:
        return None, ()
    thr = np.searchsorted(hi, np.arange(1, bins.size + 1), side="left")
    return thr.astype(np.int32), tuple(int(a) for a in amb)


def finish_bins(cnt, s1, s2, boxfactor, eps=0.):
    """(mean, std/sqrt(n)) per bin from (count, sum |dk|^2, sum |dk|^4), bin 0 dropped (box.py:761-768); NaN for empty
    bins.  ``eps``: rounding unit of the |dk|^2 values the sums were formed from (2^-23 for a single-precision plan).
    A bin that holds one mode and its mirror image (count 2: the same |dk|^2 twice for a real field), or a single
    self-mirrored mode (count 1: a corner of the grid), has exactly 0 spread in the reference's np.std; the form
    sum p^2 - (sum p)^2 / n leaves +-eps p^2 of rounding there instead, whose square root would read as a spread of
    2e-4 -- so for such bins, and only there, a variance below 4 eps mean^2 is reported as 0.  Every other bin gets the variance its sums give (a spread below ~sqrt(eps) of the
    mean is beyond what sums of single-precision squares resolve; the fp64 plan resolves 1e-8)."""
    with np.errstate(all="ignore"):
        vals = s1 / (cnt * boxfactor)
        var = (s2 - s1 * s1 / cnt) / cnt
        if eps:
            var = np.where((cnt <= 2) & (var <= 4. * eps * (s1 / cnt) ** 2), 0., var)
        stddev = np.sqrt(np.maximum(var, 0.)) / boxfactor / np.sqrt(cnt)
    return np.array(vals[1:]), np.array(stddev[1:])


def bin_counts(N, Lside, bins):
    """Number of modes of the full (N,N,N) grid per np.digitize index (host, cubic boxes): used
    when no device is at hand (tests of the slab driver)."""
    m = mode_numbers(N)
    a = (m / Lside) ** 2.
    k = 2. * np.pi * np.sqrt(a[:, None, None] + a[None, :, None] + a[None, None, :])
    idx = np.digitize(k.ravel(), bins)
    return np.bincount(idx, minlength=bins.size + 1)[:bins.size].astype(np.float64)


# ---- two-point correlation function (CosmoBox.correlation_function) ------------------------------------------------------
POLES = (0, 2, 4)
SEP_MAX_BINS = 1024          # FB_MAX_SEP_BINS of the library: dr = L/N up to rmax = L/2 at N = 2048


def separation_edges(L, N, dr=None, rmin=0., rmax=None, rbins=None):
    """Bin edges in separation: ``rbins`` as given, or np.arange(rmin, rmax + dr/2, dr) with dr = min(L_a)/N and
    rmax = min(L_a)/2 by default (nbodykit's FFTCorr(dr=, rmin=, rmax=) grid).  Strictly ascending, first edge >= 0,
    at least one bin and at most 1024 (the default edges of a 2048^3 box); ValueError otherwise."""
    if rbins is not None:
        edges = np.array(rbins, dtype=np.float64)
    else:
        lmin = float(np.min(L))
        dr = lmin / N if dr is None else float(dr)
        rmax = 0.5 * lmin if rmax is None else float(rmax)
        if not dr > 0:
            raise ValueError("dr must be positive")
        edges = np.arange(float(rmin), rmax + 0.5 * dr, dr, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges.size > SEP_MAX_BINS + 1:
        raise ValueError("separation bins: between 2 and %d edges (1 to %d bins), got %r"
                         % (SEP_MAX_BINS + 1, SEP_MAX_BINS, edges.shape))
    if not np.all(np.isfinite(edges[:-1])) or not edges[0] >= 0. or not np.all(np.diff(edges) > 0):
        raise ValueError("separation bin edges must be strictly ascending and start at >= 0")
    return edges


def check_poles(poles):
    """The multipoles asked for as a tuple of ints out of (0, 2, 4); None -> (0,)."""
    if poles is None:
        return (0,)
    ps = tuple(int(p) for p in np.atleast_1d(poles))
    if not ps or any(p not in POLES for p in ps) or any(float(p) != q for p, q in zip(ps, np.atleast_1d(poles))):
        raise ValueError("poles must be a subset of (0, 2, 4), got %r" % (poles,))
    return ps


def finish_correlation(raw, nbins, poles):
    """(r, xi, npairs) from fb_bin_separation's record [npairs, sum |s|, sum xi L_l for l = 0, 2, .. lmax]:
    r = mean |s| per bin (nbodykit's r column), xi_l = (2l + 1) sum xi L_l / npairs; empty bins NaN."""
    raw = np.asarray(raw, dtype=np.float64)
    npairs = raw[:nbins].copy()
    with np.errstate(all="ignore"):
        empty = npairs == 0
        r = np.where(empty, np.nan, raw[nbins:2 * nbins] / npairs)
        xi = np.array([np.where(empty, np.nan, (2 * l + 1) * raw[(2 + l // 2) * nbins:(3 + l // 2) * nbins] / npairs)
                       for l in poles])
    return r, xi, npairs


# ---- power spectrum in (k, mu) bins (CosmoBox.power_spectrum) -------------------------------------------------------------
PK_MAX_K = 1024              # FB_PK_MAX_K of the library: dk = 2 pi / L up to Nyquist at N = 2048
PK_MAX_MU = 128              # FB_PK_MAX_MU
PK_MAX_VALUES = 5120         # FB_PK_MAX_VALUES: nk * Nmu * (lmax / 2 + 1), one wave's 40 KiB LDS row (1024 x 5)


def power_edges(L, N, dk=None, kmin=0., kmax=None, kbins=None):
    """Bin edges in |k|: ``kbins`` as given, or np.arange(kmin, kmax + dk/2, dk) with dk = 2 pi / min(L_a) and
    kmax = pi N / max(L_a) (the coarsest axis's Nyquist) by default -- nbodykit's FFTPower(dk=, kmin=, kmax=) grid, N/2 bins
    on a cube.  Strictly ascending, first edge >= 0, all finite but the last, 1 to 1024 bins; ValueError otherwise."""
    if kbins is not None:
        edges = np.array(kbins, dtype=np.float64)
    else:
        dk = 2. * np.pi / float(np.min(L)) if dk is None else float(dk)
        kmax = np.pi * N / float(np.max(L)) if kmax is None else float(kmax)
        if not dk > 0:
            raise ValueError("dk must be positive")
        edges = np.arange(float(kmin), kmax + 0.5 * dk, dk, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges.size > PK_MAX_K + 1:
        raise ValueError("k bins: between 2 and %d edges (1 to %d bins), got %r" % (PK_MAX_K + 1, PK_MAX_K, edges.shape))
    if not np.all(np.isfinite(edges[:-1])) or not edges[0] >= 0. or not np.all(np.diff(edges) > 0):
        raise ValueError("k bin edges must be strictly ascending and start at >= 0")
    return edges


def mu_edges(Nmu):
    """np.linspace(0, 1, Nmu + 1): nbodykit's mu bins (mu = 1 counted in the last); 1 <= Nmu <= 128, ValueError otherwise."""
    if isinstance(Nmu, bool) or not isinstance(Nmu, (int, np.integer)) or not 1 <= Nmu <= PK_MAX_MU:
        raise ValueError("Nmu must be an integer in 1..%d, got %r" % (PK_MAX_MU, Nmu))
    return np.linspace(0., 1., int(Nmu) + 1)


def check_power_layout(nk, nmu, lmax):
    """ValueError unless nk * nmu * (lmax / 2 + 1) fits one wave's LDS row of the binning kernel."""
    if nk * nmu * (lmax // 2 + 1) > PK_MAX_VALUES:
        raise ValueError("%d k bins x %d mu bins x %d multipoles: at most %d cells x multipoles"
                         % (nk, nmu, lmax // 2 + 1, PK_MAX_VALUES))


def finish_power(raw, nk, nmu, poles=None):
    """From fb_bin_power_kmu's record [modes, sum |k|, sum mu, sum P (nk * nmu each); sum P L_l (nk each), l = 2, .. lmax]:
    (k, mu, power, modes), each (nk, nmu), with k, mu, power the means per cell (NaN where modes is 0); with ``poles``,
    power is instead (len(poles), nk) of P_l = (2l + 1) sum P L_l / modes over each k bin (nmu must then be 1)."""
    raw = np.asarray(raw, dtype=np.float64)
    nc = nk * nmu
    modes, sk, smu, sp = (raw[q * nc:(q + 1) * nc].reshape(nk, nmu).copy() for q in range(4))
    with np.errstate(all="ignore"):
        empty = modes == 0
        k = np.where(empty, np.nan, sk / modes)
        mu = np.where(empty, np.nan, smu / modes)
        if poles is None:
            return k, mu, np.where(empty, np.nan, sp / modes), modes
        assert nmu == 1
        m1, e1 = modes[:, 0], empty[:, 0]
        sums = {0: sp[:, 0]}
        for q, l in enumerate((2, 4)):
            lo = 4 * nc + q * nk
            if raw.size >= lo + nk:
                sums[l] = raw[lo:lo + nk]
        power = np.array([np.where(e1, np.nan, (2 * l + 1) * sums[l] / m1) for l in poles])
    return k, mu, power, modes


# ---- cylindrical power and multi-frequency angular power (CosmoBox.cylindrical_power_spectrum, .angular_power_spectrum) ------
CYL_MAX_PERP = 1024          # FB_CYL_MAX_PERP of the library: dk_perp = 2 pi / L up to Nyquist at N = 2048
CYL_MAX_PAR = 1025           # FB_CYL_MAX_PAR: one bin per |m_z| at N = 2048
MAPS_MAX_BINS = 256          # FB_MAPS_MAX_BINS
MAPS_MAX_N = 1024            # FB_MAPS_MAX_N


def _perp_edges(L, N, kperp_bins, dk_perp, kperp_min, kperp_max, most):
    """k_perp edges: ``kperp_bins`` as given, or np.arange(kperp_min, kperp_max + dk_perp/2, dk_perp) with
    dk_perp = 2 pi / min(Lx, Ly) and kperp_max = pi N / max(Lx, Ly) by default.  The checks and messages of power_edges."""
    if kperp_bins is not None:
        edges = np.array(kperp_bins, dtype=np.float64)
    else:
        dk = 2. * np.pi / float(min(L[0], L[1])) if dk_perp is None else float(dk_perp)
        kmax = np.pi * N / float(max(L[0], L[1])) if kperp_max is None else float(kperp_max)
        if not dk > 0:
            raise ValueError("dk must be positive")
        edges = np.arange(float(kperp_min), kmax + 0.5 * dk, dk, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges.size > most + 1:
        raise ValueError("k bins: between 2 and %d edges (1 to %d bins), got %r" % (most + 1, most, edges.shape))
    if not np.all(np.isfinite(edges[:-1])) or not edges[0] >= 0. or not np.all(np.diff(edges) > 0):
        raise ValueError("k bin edges must be strictly ascending and start at >= 0")
    return edges


def cyl_edges(L, N, kperp_bins=None, kpar_bins=None, dk_perp=None, kperp_min=0., kperp_max=None):
    """(k_perp edges, k_par edges) of the cylindrical power spectrum.  k_perp: ``kperp_bins``, or
    np.arange(kperp_min, kperp_max + dk_perp/2, dk_perp) with dk_perp = 2 pi / min(Lx, Ly), kperp_max = pi N / max(Lx, Ly);
    strictly ascending, first edge >= 0, all finite but the last, 1 to 1024 bins.  k_par: ``kpar_bins``, or one bin around
    every |m_z|, (np.arange(N/2 + 2) - 0.5) 2 pi / Lz (N/2 + 1 bins); strictly ascending, all finite but the last (the first
    may be negative: k_par = |k_z| >= 0 anyway), 1 to 1025 bins.  ValueError otherwise."""
    perp = _perp_edges(L, N, kperp_bins, dk_perp, kperp_min, kperp_max, CYL_MAX_PERP)
    if kpar_bins is not None:
        par = np.array(kpar_bins, dtype=np.float64)
    else:
        par = (np.arange(N // 2 + 2) - 0.5) * (2. * np.pi / float(L[2]))
    if par.ndim != 1 or par.size < 2 or par.size > CYL_MAX_PAR + 1:
        raise ValueError("k bins: between 2 and %d edges (1 to %d bins), got %r" % (CYL_MAX_PAR + 1, CYL_MAX_PAR, par.shape))
    if not np.all(np.isfinite(par[:-1])) or not np.all(np.diff(par) > 0):
        raise ValueError("k_par bin edges must be strictly ascending")
    return perp, par


def maps_edges(L, N, kperp_bins=None, dk_perp=None, kperp_min=None, kperp_max=None):
    """k_perp edges of the multi-frequency angular power spectrum: as cyl_edges, but starting at half the fundamental
    (kperp_min = pi / min(Lx, Ly)) by default, 1 to 256 bins, and N <= 1024.  ValueError otherwise."""
    if N > MAPS_MAX_N:
        raise ValueError("angular_power_spectrum: grids up to %d^3" % MAPS_MAX_N)
    if kperp_min is None:
        kperp_min = np.pi / float(min(L[0], L[1]))
    return _perp_edges(L, N, kperp_bins, dk_perp, kperp_min, kperp_max, MAPS_MAX_BINS)


def finish_cyl(raw, nperp, npar):
    """From fb_bin_power_cyl's record [modes, sum k_perp, sum k_par, sum P (nperp * npar each)]: (kperp, kpar, power, modes),
    each (nperp, npar), the first three the means per cell (NaN where modes is 0)."""
    raw = np.asarray(raw, dtype=np.float64)
    nc = nperp * npar
    modes, sperp, spar, sp = (raw[q * nc:(q + 1) * nc].reshape(nperp, npar).copy() for q in range(4))
    with np.errstate(all="ignore"):
        empty = modes == 0
        return (np.where(empty, np.nan, sperp / modes), np.where(empty, np.nan, spar / modes),
                np.where(empty, np.nan, sp / modes), modes)


def finish_maps(raw, nb):
    """From fb_transverse_gram's record [modes, sum k_perp (nb each)]: (kperp (nb,) float64, the mean per bin, NaN where the
    bin is empty; modes (nb,) int64)."""
    raw = np.asarray(raw, dtype=np.float64)
    modes, sk = raw[:nb], raw[nb:2 * nb]
    with np.errstate(all="ignore"):
        kperp = np.where(modes == 0, np.nan, sk / modes)
    return kperp, np.rint(modes).astype(np.int64)


def collapse_maps(cl):
    """(nb, N) from (nb, N, N): out[b, D] = the mean of cl[b, nu, nu + D] over the N - D pairs of channels D apart."""
    cl = np.asarray(cl, dtype=np.float64)
    if cl.ndim != 3 or cl.shape[1] != cl.shape[2]:
        raise ValueError("collapse_maps: expected an array of shape (nb, N, N), got %r" % (cl.shape,))
    N = cl.shape[1]
    return np.stack([np.trace(cl, offset=D, axis1=1, axis2=2) / float(N - D) for D in range(N)], axis=1)


# ---- bispectrum in triangle bins (CosmoBox.bispectrum) ---------------------------------------------------------------------
BK_MAX_SHELLS = 32           # FB_BK_MAX_SHELLS of the library: two 16-row tiles of the contraction
BK_DEFAULT_SHELLS = 16


def bispectrum_edges(L, N, dk=None, kmin=0., kmax=None, kbins=None):
    """Shell edges in |k|: ``kbins`` as given; with ``dk`` np.arange(kmin, kmax + dk/2, dk); otherwise
    np.linspace(kmin, kmax, 17) (16 shells).  kmax = (2/3) pi N / max(L_a) by default: below it no triangle closes through
    an alias.  Strictly ascending, first edge >= 0, all finite but the last, 1 to 32 shells; ValueError otherwise."""
    if kbins is not None:
        if dk is not None:
            raise ValueError("give kbins or dk, not both")
        edges = np.array(kbins, dtype=np.float64)
    else:
        kmax = (2. / 3.) * np.pi * N / float(np.max(L)) if kmax is None else float(kmax)
        if dk is None:
            edges = np.linspace(float(kmin), kmax, BK_DEFAULT_SHELLS + 1)
        else:
            dk = float(dk)
            if not dk > 0:
                raise ValueError("dk must be positive")
            if not (kmax - float(kmin)) / dk <= 4 * BK_MAX_SHELLS:         # (refused below; never build a huge arange)
                raise ValueError("k shells: at most %d" % BK_MAX_SHELLS)
            edges = np.arange(float(kmin), kmax + 0.5 * dk, dk, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2 or edges.size > BK_MAX_SHELLS + 1:
        raise ValueError("k shells: between 2 and %d edges (1 to %d shells), got %r"
                         % (BK_MAX_SHELLS + 1, BK_MAX_SHELLS, edges.shape))
    if not np.all(np.isfinite(edges[:-1])) or np.isnan(edges[-1]) or not edges[0] >= 0. or not np.all(np.diff(edges) > 0):
        raise ValueError("k shell edges must be strictly ascending and start at >= 0")
    return edges


def bispectrum_triples(nb):
    """(T, 3) shell indices b1 <= b2 <= b3 in itertools.combinations_with_replacement(range(nb), 3) order,
    T = nb (nb + 1) (nb + 2) / 6."""
    import itertools
    if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or not 1 <= nb <= BK_MAX_SHELLS:
        raise ValueError("the number of shells must be an integer in 1..%d, got %r" % (BK_MAX_SHELLS, nb))
    return np.array(list(itertools.combinations_with_replacement(range(int(nb)), 3)), dtype=np.intp).reshape(-1, 3)


def bispectrum_ntri(raw, nb, N):
    """Closed triangles per triple from the record of a unit-spectrum pass of fb_bispectrum (sum_x U_b1 U_b2 U_b3 = N^3
    ntri, formed in fp64): rounded to the nearest integer."""
    T = nb * (nb + 1) * (nb + 2) // 6
    return np.rint(np.asarray(raw, dtype=np.float64)[:T] / float(N) ** 3)


def finish_bispectrum(raw, ntri, nb, L, N):
    """From fb_bispectrum's record [sum_x I_b1 I_b2 I_b3 (T); modes, sum |k|, sum |D|^2 (nb each)] and the triangle counts:
    (k (T, 3), B (T,), Q (T,), ntri (T,)) with B = (V^2 / N^12) sum / ntri, k the mean |k| of each triple's shells,
    Q = B / (P1 P2 + P2 P3 + P3 P1), P_b = (V / N^6) sum |D|^2 / modes.  Triples without a triangle are NaN in k, B and Q;
    an empty shell has mean |k| NaN."""
    raw = np.asarray(raw, dtype=np.float64)
    tri = bispectrum_triples(nb)
    T = tri.shape[0]
    sums = raw[:T]
    modes, sk, sp = (raw[T + q * nb:T + (q + 1) * nb] for q in range(3))
    ntri = np.array(ntri, dtype=np.float64)
    n3 = float(N) ** 3
    V = float(L[0]) * float(L[1]) * float(L[2])
    with np.errstate(all="ignore"):
        kbar = np.where(modes == 0, np.nan, sk / modes)
        P = np.where(modes == 0, np.nan, (V / (n3 * n3)) * sp / modes)
        empty = ntri == 0
        B = np.where(empty, np.nan, ((V * V) / n3 ** 4) * sums / ntri)
        k = kbar[tri]
        k[empty] = np.nan
        p1, p2, p3 = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
        Q = B / (p1 * p2 + p2 * p3 + p3 * p1)
    return k, B, Q, ntri
