"""Constructed inputs for the binning kernels (fb_bin_power, fb_bin_power_filtered, fb_bin_power_kmu, fb_bin_power_cyl,
fb_bin_separation, fb_cross_power_half, fb_transverse_gram) with references that hold bit for bit.

Stored spectra, real fields and transverse cubes are fixed arithmetic patterns of the indices with |re|, |im| <= 15 (no RNG: within
a row every stored mode has its own (re, im) pair), so |D|^2 <= 450 is exact in fp32 and every product and every partial sum a
kernel forms is an integer far below 2^53: whatever the summation order, a correct device sum EQUALS the np.bincount one.  The
spectra are deliberately not Hermitian -- a binning kernel bins what is stored.  The padding columns and the spare row of every
half-layout array hold NaN: the kernels document that they read neither.

Cell membership is taken from tests/pk_numpy.py, cyl_numpy.py and corrfn_numpy.py where they state it; the shell binning of
fb_bin_power (thresholds and ambiguous shells as CosmoBox hands them over, the exact |k| elsewhere) is stated here.  Sums with
non-integer weights (|k|, mu, |s|, Legendre multipoles) are formed term by term in np.longdouble and added with math.fsum.
The wavenumber tables, the wedge's k_par and the shell thresholds of the fb_bin_power references come from fastbox_amd.hostgeom,
the tables the engine itself uploads (with the reference's integer truncation of fftfreq at N = 18 and 24, where mode 7 becomes
0): these cases show that the kernels bin by the project's tables, not that the tables are right -- that is what the random-field
tests against pk_numpy.py, cyl_numpy.py and corrfn_numpy.py (test_power_spectrum_gpu.py, test_box_gpu.py, ...) are for.
The branch predicates at the end restate, from the sources, the launch decisions a case is meant to reach;
tests/test_binning_cases_cpu.py asserts them."""
import math

import numpy as np

from fastbox_amd import hostgeom
from tests import corrfn_numpy as cf
from tests import cyl_numpy as cn
from tests import pk_numpy as pk

EXACT = 2 ** 53
U = 2. ** -53
CUBOID = (100., 130., 170.)
STANDARD = [(16, 100.), (18, 100.), (24, 100.), (16, CUBOID)]          # the geometries every kernel is run on


def sides(L):
    return tuple(float(x) for x in L) if isinstance(L, tuple) else (float(L),) * 3


def box_scale(L):
    """The box_scale argument of CosmoBox for these side lengths."""
    L = sides(L)
    return L[0] if L[0] == L[1] == L[2] else L


def half_dims(N):
    """(stored k_z, rows per x-plane, row pitch) of a stored half spectrum."""
    return N // 2 + 1, N + 1, (N // 2 + 1 + 15) & ~15


# ---- the integer patterns ------------------------------------------------------------------------------------------------------
# (a, b, c, offset, modulus, shift): value = (a i + b j + c l + offset) % modulus - shift.  The l coefficients are units modulo
# 31 and 29: the (re, im) pairs of a row repeat only after 31 * 29 = 899 elements.
PATTERNS = (((7, 13, 29, 0, 31, 15), (11, 5, 17, 3, 29, 14)),           # first operand
            ((5, 11, 23, 7, 31, 15), (13, 7, 19, 5, 29, 14)))          # second (cross) operand


def ints(N, nz, which, i0, i1=None):
    """(re, im) int64 [i1 - i0][N][nz]: x-planes i0 .. i1 - 1 of pattern `which`."""
    i1 = i0 + 1 if i1 is None else i1
    i = np.arange(i0, i1, dtype=np.int64)[:, None, None]
    j = np.arange(N, dtype=np.int64)[None, :, None]
    l = np.arange(nz, dtype=np.int64)[None, None, :]
    return tuple((a * i + b * j + c * l + o) % m - s for a, b, c, o, m, s in PATTERNS[which])


def _fill(view, N, nz, which):
    step = max(1, (1 << 22) // (N * nz))
    for i0 in range(0, N, step):
        re, im = ints(N, nz, which, i0, min(N, i0 + step))
        v = view[i0:i0 + step]
        v.real = re
        v.imag = im


def stored_half(N, which, cdtype, poison=complex(np.nan, np.nan)):
    """[N][N + 1][pitch] as the plan stores a half spectrum; padding columns and the spare row hold `poison`."""
    nzv, nr, nzp = half_dims(N)
    a = np.full((N, nr, nzp), poison, dtype=cdtype)
    _fill(a[:, :N, :nzv], N, nzv, which)
    return a


def stored_full(N, which, cdtype):
    a = np.empty((N, N, N), dtype=cdtype)
    _fill(a, N, N, which)
    return a


def real_field(N, which, rdtype):
    return ints(N, N, which, 0, N)[0].astype(rdtype)


TABLE_VALUES = np.array([0., 0.5, 1., 2.])


def table_ints(N, nz, i0, i1=None):
    i1 = i0 + 1 if i1 is None else i1
    i = np.arange(i0, i1, dtype=np.int64)[:, None, None]
    return (3 * i + 5 * np.arange(N, dtype=np.int64)[None, :, None] + 7 * np.arange(nz, dtype=np.int64)[None, None, :]) % 4


def filter_table(N, layout, rdtype):
    """A real multiplier with entries in {0, 0.5, 1, 2} in the layout of the field (half: padding poisoned)."""
    if layout == "full":
        return TABLE_VALUES[table_ints(N, N, 0, N)].astype(rdtype)
    nzv, nr, nzp = half_dims(N)
    t = np.full((N, nr, nzp), np.nan, dtype=rdtype)
    t[:, :N, :nzv] = TABLE_VALUES[table_ints(N, nzv, 0, N)]
    return t


# ---- exact sums of extended-precision terms ------------------------------------------------------------------------------------
class CellSums(object):
    """sum of np.longdouble terms per cell with math.fsum.  A term is split into its double and the remainder; the doubles of a
    cell are added exactly (fsum), the remainders (2^-53 of the terms) in extended precision.  Terms are buffered up to `limit`;
    every case up to 128^3 is one batch, so its sums are the correctly rounded ones.  A 512^3 case is flushed every few planes:
    a cell's batch sums are each rounded once and then added exactly, an error below 2^-53 sum |term| -- one unit of the
    n_b + 64 (or n_b + 8) the bounds allow, not added to them."""

    def __init__(self, nc, limit=1 << 23):
        self.nc, self.limit, self.held = nc, limit, 0
        self.buf, self.parts = [], [[] for _ in range(nc)]

    def add(self, cell, term):
        self.buf.append((np.asarray(cell).ravel(), np.asarray(term, dtype=np.longdouble).ravel()))
        self.held += self.buf[-1][0].size
        if self.held >= self.limit:
            self.flush()

    def flush(self):
        if not self.buf:
            return
        cell = np.concatenate([b[0] for b in self.buf])
        term = np.concatenate([b[1] for b in self.buf])
        self.buf, self.held = [], 0
        order = np.argsort(cell, kind="stable")
        cell, term = cell[order], term[order]
        hi = term.astype(np.float64)
        lo = (term - hi).astype(np.float64)
        cut = np.searchsorted(cell, np.arange(self.nc + 1))
        hl, ll = hi.tolist(), lo.tolist()
        for c in np.nonzero(np.diff(cut))[0]:
            self.parts[c].append(math.fsum(hl[cut[c]:cut[c + 1]]))
            self.parts[c].append(math.fsum(ll[cut[c]:cut[c + 1]]))

    def result(self):
        self.flush()
        return np.array([math.fsum(p) for p in self.parts])


def legendre_ld(l, m2):
    m2 = np.asarray(m2, dtype=np.longdouble)
    if l == 2:
        return np.longdouble(1.5) * m2 - np.longdouble(0.5)
    if l == 4:
        return ((35 * m2 - 30) * m2 + 3) * np.longdouble(0.125)
    raise ValueError(l)


# ---- fb_bin_power / fb_bin_power_filtered --------------------------------------------------------------------------------------
def shell_setup(N, L, edges):
    """(thr, amb) as CosmoBox._bin_setup hands them to Engine.set_bins: integer-shell thresholds on a cube (None when more than
    8 shells lie within rounding of an edge), None on any other box."""
    L = sides(L)
    if not (L[0] == L[1] == L[2]):
        return None, ()
    return hostgeom.shell_thresholds(N, L[0], np.asarray(edges, dtype=np.float64))


def kmag_planes(N, L, nz, i0, i1):
    """|k| of box.py:125-131, the expression the kernels evaluate where they need the exact value."""
    a2 = hostgeom.axis_tables(N, sides(L))[0]
    s = (a2[i0:i1, None, None] + a2[N:2 * N][None, :, None]) + a2[2 * N:2 * N + nz][None, None, :]
    return 2. * np.pi * np.sqrt(s)


def power_bins(N, L, edges, layout, i0, i1):
    """np.digitize bin (0 .. nbins; nbins = beyond the last edge, dropped) of x-planes i0 .. i1 - 1 as the header defines it:
    the step function of the integer shell n^2 where thresholds are in use, the exact |k| for the ambiguous shells and on
    every box without thresholds."""
    edges = np.asarray(edges, dtype=np.float64)
    nz = N if layout == "full" else N // 2 + 1
    thr, amb = shell_setup(N, L, edges)
    if thr is None:
        return np.digitize(kmag_planes(N, L, nz, i0, i1), edges)
    m = pk.signed_index(N)
    n2 = m[i0:i1, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :nz] ** 2
    b = np.searchsorted(thr, n2, side="right")
    if len(amb):
        sel = np.isin(n2, amb)
        b[sel] = np.digitize(kmag_planes(N, L, nz, i0, i1)[sel], edges)
    return b


def mode_weight(N, layout):
    """Multiplicity of a stored mode in the full grid."""
    if layout == "full":
        return np.ones(N)
    l = np.arange(N // 2 + 1)
    return np.where((l == 0) | (2 * l == N), 1., 2.)


def filter_multiplier(N, L, layout, filt, i0, i1):
    """The real multiplier T(k_perp, k_par) of x-planes i0 .. i1 - 1; filt: None, ('wedge', slope, offset) or ('table',)."""
    nz = N if layout == "full" else N // 2 + 1
    if filt is None:
        return np.ones((i1 - i0, N, nz))
    if filt[0] == "table":
        return TABLE_VALUES[table_ints(N, nz, i0, i1)]
    a2, _, kpar = hostgeom.axis_tables(N, sides(L))
    kperp = 2. * np.pi * np.sqrt(a2[i0:i1, None] + a2[N:2 * N][None, :])
    edge = filt[1] * kperp + filt[2]                                  # product and sum rounded separately, as numpy does
    return np.where(np.abs(kpar[:nz])[None, None, :] < edge[:, :, None], 0., 1.)


def ref_bin_power(N, L, edges, layout, filt=None, which=0):
    """(count, sum, sumsq) [nbins] of fb_bin_power / fb_bin_power_filtered, every entry an exact dyadic number."""
    nb = np.asarray(edges).size
    nz = N if layout == "full" else N // 2 + 1
    w = mode_weight(N, layout)[None, None, :]
    out = np.zeros((3, nb + 1))
    step = max(1, (1 << 21) // (N * nz))
    for i0 in range(0, N, step):
        i1 = min(N, i0 + step)
        re, im = ints(N, nz, which, i0, i1)
        t = filter_multiplier(N, L, layout, filt, i0, i1)
        p = (re * re + im * im) * (t * t)
        b = power_bins(N, L, edges, layout, i0, i1).ravel()
        for q, v in enumerate((w * np.ones_like(p), w * p, w * p * p)):
            out[q] += np.bincount(b, weights=v.ravel(), minlength=nb + 1)
    assert np.all(out < EXACT)
    return out[0, :nb], out[1, :nb], out[2, :nb]


# ---- fb_bin_power_kmu ----------------------------------------------------------------------------------------------------------
def power_scale(N, L):
    """Lx Ly Lz / N^6, the double bin_power_kmu and bin_power_cyl form."""
    L = sides(L)
    n3 = float(N) * N * N
    return (L[0] * L[1] * L[2]) / (n3 * n3)


def cross_ints(N, nz, cross, i0, i1=None):
    """Re(conj(D_1) D_2) of x-planes i0 .. i1 - 1 (int64)."""
    re, im = ints(N, nz, 0, i0, i1)
    if not cross:
        return re * re + im * im
    r2, i2 = ints(N, nz, 1, i0, i1)
    return re * r2 + im * i2


def ref_kmu(N, L, kedges, nmu, lmax, cross=False):
    """Per cell [nk nmu]: modes, terms (stored modes), sum_int (sum w Re(conj D_1 D_2), an integer), sum_abs (sum w |p|),
    sum_k, sum_mu (extended precision) and the sums w |k|, w mu of the bounds; per k bin [nk]: terms_k, abs_k and
    poles {l: sum w p L_l(mu)} (extended precision)."""
    L = sides(L)
    kedges = np.asarray(kedges, dtype=np.float64)
    nk, nz = kedges.size - 1, N // 2 + 1
    nc = nk * nmu
    kx, ky, kz = pk.wavenumbers(N, L)
    kzh = kz[:nz]
    w = mode_weight(N, "half")[None, :] * np.ones((N, 1))
    ld = np.longdouble
    kyl, kzl = ky.astype(ld), kzh.astype(ld)
    out = {k: np.zeros(nc) for k in ("modes", "terms", "sum_int", "sum_abs")}
    sk, smu = CellSums(nc), CellSums(nc)
    poles = {l: CellSums(nk) for l in range(2, lmax + 1, 2)}
    for i in range(N):
        K = np.sqrt((kx[i] * kx[i] + ky[:, None] * ky[:, None]) + kzh[None, :] * kzh[None, :])
        with np.errstate(invalid="ignore", divide="ignore"):
            mu = np.where(K > 0, np.abs(kzh)[None, :] / K, 0.)
        cell, ok = pk._bin_cells(K, mu, kedges, nmu)
        c = cell[ok]
        p = cross_ints(N, nz, cross, i)[0]
        for key, v in (("modes", w), ("terms", np.ones_like(w)), ("sum_int", w * p), ("sum_abs", w * np.abs(p))):
            out[key] += np.bincount(c, weights=v[ok], minlength=nc)
        k2 = (ld(kx[i]) * ld(kx[i]) + kyl[:, None] * kyl[:, None]) + kzl[None, :] * kzl[None, :]
        k2 = k2[ok]
        kzo = np.broadcast_to(kzl[None, :], w.shape)[ok]
        Kl = np.sqrt(k2)
        sk.add(c, w[ok] * Kl)
        smu.add(c, w[ok] * (np.abs(kzo) / Kl))
        if lmax:
            m2 = (kzo * kzo) / k2
            for l in poles:
                poles[l].add(c // nmu, (w * p)[ok] * legendre_ld(l, m2))
    assert np.all(out["sum_abs"] < EXACT)
    out["sum_k"], out["sum_mu"] = sk.result(), smu.result()
    out["poles"] = {l: s.result() for l, s in poles.items()}
    out["terms_k"] = out["terms"].reshape(nk, nmu).sum(axis=1)
    out["abs_k"] = out["sum_abs"].reshape(nk, nmu).sum(axis=1)
    return out


# ---- fb_bin_power_cyl ----------------------------------------------------------------------------------------------------------
def perp_bins(N, L, perp_edges):
    """(k_perp [N][N], bin or -1) of the transverse plane."""
    kp = cn.kperp_plane(N, sides(L))
    b, ok = cn._digitize(kp, np.asarray(perp_edges, dtype=np.float64))
    return kp, np.where(ok, b, -1)


def ref_cyl(N, L, perp_edges, par_edges, cross=False, wavenumbers=True):
    """Per cell [nperp npar]: modes, terms, sum_int, sum_abs and, with `wavenumbers`, sum_kperp, sum_kpar (extended precision;
    the library forms these two on the host, no kernel is involved)."""
    L = sides(L)
    pe, qe = np.asarray(perp_edges, dtype=np.float64), np.asarray(par_edges, dtype=np.float64)
    nperp, npar, nz = pe.size - 1, qe.size - 1, N // 2 + 1
    nc = nperp * npar
    kp, b = perp_bins(N, L, pe)
    kq = np.abs(pk.wavenumbers(N, L)[2][:nz])
    c, okc = cn._digitize(kq, qe)
    w = mode_weight(N, "half")[None, :] * np.ones((N, 1))
    out = {k: np.zeros(nc) for k in ("modes", "terms", "sum_int", "sum_abs")}
    sp, sq = CellSums(nc), CellSums(nc)
    for i in range(N):
        ok = (b[i] >= 0)[:, None] & okc[None, :] & ((kp[i][:, None] > 0) | (kq[None, :] > 0))
        cell = (b[i][:, None] * npar + c[None, :])[ok]
        p = cross_ints(N, nz, cross, i)[0]
        for key, v in (("modes", w), ("terms", np.ones_like(w)), ("sum_int", w * p), ("sum_abs", w * np.abs(p))):
            out[key] += np.bincount(cell, weights=v[ok], minlength=nc)
        if wavenumbers:
            sp.add(cell, (w * kp[i][:, None].astype(np.longdouble))[ok])
            sq.add(cell, (w * kq[None, :].astype(np.longdouble))[ok])
    assert np.all(out["sum_abs"] < EXACT)
    if wavenumbers:
        out["sum_kperp"], out["sum_kpar"] = sp.result(), sq.result()
    return out


# ---- fb_bin_separation ---------------------------------------------------------------------------------------------------------
def ref_separation(N, L, edges, lmax, which=0):
    """Per bin: npairs, sum_int (sum xi), sum_abs (sum |xi|), sum_r and poles {l: sum xi L_l(mu)} (extended precision)."""
    L = sides(L)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    xi = ints(N, N, which, 0, N)[0]
    m = cf.signed_index(N)
    sx, sy, sz = [m * (La / N) for La in L]
    sx, sy, sz = sx[:, None, None], sy[None, :, None], sz[None, None, :]
    S = np.sqrt((sx * sx + sy * sy) + sz * sz)
    b = np.digitize(S, edges) - 1
    ok = (b >= 0) & (b < nb)
    bv = b[ok]
    out = dict(npairs=np.bincount(bv, minlength=nb).astype(np.float64),
               sum_int=np.bincount(bv, weights=xi[ok].astype(np.float64), minlength=nb),
               sum_abs=np.bincount(bv, weights=np.abs(xi[ok]).astype(np.float64), minlength=nb))
    assert np.all(out["sum_abs"] < EXACT)
    ld = np.longdouble
    sxl, syl, szl = sx.astype(ld), sy.astype(ld), sz.astype(ld)
    S2 = ((sxl * sxl + syl * syl) + szl * szl)[ok]
    sr = CellSums(nb)
    sr.add(bv, np.sqrt(S2))
    out["sum_r"] = sr.result()
    out["poles"] = {}
    if lmax:
        szo = np.broadcast_to(szl, S.shape)[ok]
        with np.errstate(invalid="ignore", divide="ignore"):
            m2 = np.where(S2 > 0, (szo * szo) / S2, ld(0))
        for l in range(2, lmax + 1, 2):
            s = CellSums(nb)
            s.add(bv, xi[ok].astype(ld) * legendre_ld(l, m2))
            out["poles"][l] = s.result()
    return out


# ---- fb_cross_power_half -------------------------------------------------------------------------------------------------------
def ref_cross_power(N, cross, scale, cdtype):
    """[N][N][N/2 + 1] conj(a) b scale (cross False: |a|^2 with imaginary part 0), k = 0 set to 0, in the plan's precision."""
    nz = N // 2 + 1
    re, im = ints(N, nz, 0, 0, N)
    if cross:
        r2, i2 = ints(N, nz, 1, 0, N)
        x, y = re * r2 + im * i2, re * i2 - im * r2
    else:
        x, y = re * re + im * im, np.zeros_like(re)
    out = np.empty((N, N, nz), dtype=cdtype)
    out.real = x * scale
    out.imag = y * scale
    out[0, 0, 0] = 0
    return out


# ---- fb_transverse_gram --------------------------------------------------------------------------------------------------------
def ref_gram(N, L, perp_edges, cross=False):
    """(modes [nb], the integer Gram sums S [nb][N][N], C = S (Lx Ly / N^4 / modes_b) formed as fb_cyl.hip forms it,
    sum_kperp in extended precision): S_b(nu, nu') = sum_{m_perp in b} Re(a_1(m_perp, nu) conj(a_2(m_perp, nu')))."""
    L = sides(L)
    pe = np.asarray(perp_edges, dtype=np.float64)
    nb = pe.size - 1
    kp, b = perp_bins(N, L, pe)
    b = b.ravel().copy()
    b[0] = -1                                                          # m_perp = 0
    re, im = [x.reshape(N * N, N).astype(np.float64) for x in ints(N, N, 0, 0, N)]
    r2, i2 = [x.reshape(N * N, N).astype(np.float64) for x in ints(N, N, 1, 0, N)] if cross else (re, im)
    n2 = float(N) * N
    norm = (L[0] * L[1]) / (n2 * n2)
    modes, S, C = np.zeros(nb), np.zeros((nb, N, N)), np.full((nb, N, N), np.nan)
    sk = CellSums(nb)
    sk.add(b[b >= 0], kp.ravel()[b >= 0].astype(np.longdouble))
    for q in range(nb):
        sel = b == q
        modes[q] = np.count_nonzero(sel)
        S[q] = re[sel].T @ r2[sel] + im[sel].T @ i2[sel]
        assert np.all(np.abs(re[sel]).T @ np.abs(r2[sel]) + np.abs(im[sel]).T @ np.abs(i2[sel]) < EXACT)
        if modes[q]:
            C[q] = S[q] * (norm / modes[q])
    return modes, S, C, sk.result()


# ---- branch predicates: the launch decisions of the sources, restated ----------------------------------------------------------
BIN_GROUP, BIN_MAXSPAN = 5, 8            # FB_BIN_GROUP, FB_BIN_MAXSPAN (fb_field_kernels.h)
PK_GROUP = 4                             # FB_PK_GROUP (fb_power.hip)
LDS_DEFAULT, LDS_CU = 64 * 1024, 160 * 1024


def bin_rows_spans(N, L, edges):
    """Per (k_x, k_y) row the number of thresholds inside its n^2 range, blo and bhi (k_bin_rows with thresholds)."""
    thr, _ = shell_setup(N, L, edges)
    m = pk.signed_index(N)
    n2row = (m[:, None] ** 2 + m[None, :] ** 2).ravel()
    blo = np.searchsorted(thr, n2row, side="right")
    bhi = np.searchsorted(thr, n2row + (N // 2) ** 2, side="right")
    return bhi - blo, blo, bhi


def bin_rows_steps(N, layout):
    nz = N if layout == "full" else N // 2 + 1
    return -(-nz // (64 * BIN_GROUP))


def pk_uniform(kedges):
    """bin_power_kmu's test for evenly spaced edges (the float guess of the bin)."""
    e = [float(x) for x in kedges]
    nk = len(e) - 1
    dk = (e[nk] - e[0]) / nk
    return bool(math.isfinite(dk) and dk > 0. and all(abs(e[q] - (e[0] + q * dk)) <= 1e-6 * dk for q in range(nk + 1)))


def pk_lds(nk, nmu, nv, waves):
    return (nk + nmu + 2) * 8 + waves * nv * nk * nmu * 8


def pk_waves(nk, nmu, nv):
    for w in (4, 3, 2):
        if pk_lds(nk, nmu, nv, w) <= LDS_CU:
            return w
    return 1


def pk_row_keys(N, L, kedges, nmu, i, j):
    """Cell key per stored k_z of row (i, j) as k_pk_bin forms it: -1 below the first edge and at k = 0, a large value beyond
    the last edge."""
    L = sides(L)
    kedges = np.asarray(kedges, dtype=np.float64)
    kx, ky, kz = pk.wavenumbers(N, L)
    kzh = kz[:N // 2 + 1]
    K = np.sqrt((kx[i] * kx[i] + ky[j] * ky[j]) + kzh * kzh)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(K > 0, np.abs(kzh) / K, 0.)
    kb = np.digitize(K, kedges) - 1
    mb = np.minimum(np.digitize(mu, np.linspace(0., 1., nmu + 1)) - 1, nmu - 1)
    key = np.where(kb >= kedges.size - 1, 1 << 30, kb * nmu + mb)
    return np.where((kb < 0) | (K == 0), -1, key), K


def pk_kperp(N, L):
    return cn.kperp_plane(N, sides(L))


def cyl_chunks(N, L, perp_edges, skip0=False, rc=None):
    """Rows per chunk of fb_bin_power_cyl (rc = max(32, ceil(N^2 / 1024))): (rc, rows per bin, the list of chunk lengths)."""
    _, b = perp_bins(N, L, perp_edges)
    b = b.ravel().copy()
    if skip0:
        b[0] = -1
    nb = np.asarray(perp_edges).size - 1
    rows = np.bincount(b[b >= 0], minlength=nb)
    rc = max(32, (N * N + 1023) // 1024) if rc is None else rc
    lengths = [min(rc, r - s) for r in rows for s in range(0, r, rc)]
    return rc, rows, lengths


def gram_chunk_rows(N, nrows, cross, num_cu):
    """Modes per chunk of transverse_gram (fb_cyl.hip): the listed modes over `slices` chunks with about 8 waves per CU over all
    block pairs, whole rank-4 updates, at least 16 modes."""
    ma = gram_shape(N)[0]
    nbs = -(-N // (16 * ma))
    npairs = nbs * nbs if cross else nbs * (nbs + 1) // 2
    slices = max(1, (8 * num_cu + npairs - 1) // npairs)
    rc = (nrows + slices - 1) // slices
    return max(16, (rc + 3) & ~3)


def sep_reach(N, L, elast):
    """M_a of fbi_sep_bin: the largest |m_a| visited per axis."""
    out = []
    for La in sides(L):
        q = math.floor(elast * float(N) / La) + 1. if math.isfinite(elast) else math.inf
        out.append(N // 2 if q >= N // 2 else int(q))
    return out


def sep_lds(nbins, nv):
    return (nbins + 1) * 8 + 4 * nv * nbins * 8


def sep_row_bins(N, L, edges, a, bq):
    """Bin per |m_z| = 0 .. N/2 of the folded row (|m_x|, |m_y|) = (a, bq)."""
    L = sides(L)
    t = np.arange(N // 2 + 1)
    s = np.sqrt(((a * (L[0] / N)) ** 2 + (bq * (L[1] / N)) ** 2) + (t * (L[2] / N)) ** 2)
    return np.digitize(s, np.asarray(edges, dtype=np.float64)) - 1


def gram_shape(N):
    """(MA, EDGE) of k_maps_gram as gram_shape chooses them."""
    return (4 if N % 64 == 0 else (2 if N % 32 == 0 else 1)), N % 16 != 0


# ---- the edge sets of the cases ------------------------------------------------------------------------------------------------
def kf(L):
    return 2. * np.pi / min(sides(L))


def edges_between(N, L):
    """fb_bin_power edges between the shells of a cube: first edge above 0, last below the corner."""
    return kf(L) * (np.arange(N // 2 + 2) + 0.5)


def edges_coarse(N, L, n):
    """n edges (n <= 256) from half a fundamental to just inside the corner of the box."""
    return np.linspace(0.5 * kf(L), 0.49 * N * np.sqrt(3.) * kf(L), n)


def edges_narrow(N, L):
    """200 narrow bins over the whole box: rows span more than FB_BIN_MAXSPAN of them."""
    return np.linspace(0.45 * kf(L), 0.5 * N * np.sqrt(3.) * kf(L) * 1.01, 200)


def edges_on_shells(N, L):
    """Edges written as the |k| of axis-aligned shells: every one of them is ambiguous (8 at most)."""
    return kf(L) * np.arange(2., 17., 2.)


def kmu_edges(N, L, kind):
    k = kf(L)
    if kind == "default":
        return hostgeom.power_edges(sides(L), N)
    if kind == "wide":                                                 # one bin over every mode but k = 0
        return np.array([0., np.inf])
    if kind == "k40":
        return np.linspace(0., 0.5 * N * k, 41)
    if kind == "uniform":                                              # first edge > 0, last below the largest |k|
        return np.linspace(1.5 * k, 0.45 * N * k, 12)
    if kind == "geometric":
        return np.geomspace(1.5 * k, 0.45 * N * k, 12)
    if kind == "k1024":
        return np.linspace(0., 0.55 * N * k, 1025)
    raise ValueError(kind)


def cyl_edges(N, L, kind):
    """(perp_edges, par_edges)."""
    k = kf(L)
    kzf = 2. * np.pi / sides(L)[2]
    par = kzf * (np.arange(N // 2 + 2) - 0.5)                          # one bin around every |m_z|
    if kind == "default":
        return k * np.arange(0., N // 2 + 1), par
    if kind == "one-row":                                              # [0, 0.5 k_f) holds the row (0, 0) alone; bin 2 is empty
        return k * np.array([0., 0.5, 1.2, 1.3, 2.5, 5.2, np.inf]), kzf * np.array([0., 0.5, 2.5, 2.6, 7.5, np.inf])
    if kind == "ring32":                                               # N = 64: the two rows at |m_perp| = 32 alone
        return k * np.array([0., 0.5, 8.5, 31.99, 32.01, np.inf]), par[::3]
    if kind == "tail":                                                 # N = 64: 2035 rows, chunks of 32 and one of 19
        return k * np.array([25.6, np.inf]), par[::5]
    raise ValueError(kind)


def sep_edges(N, L, kind):
    Lm = max(sides(L))
    if kind == "all":                                                  # last edge beyond the half diagonal of the box
        return np.linspace(0., 0.9 * Lm, 13)
    if kind == "short":
        return np.linspace(0.5 * min(sides(L)) / N, min(sides(L)) / 8., 9)
    if kind == "wide":
        return np.array([0., np.inf])
    if kind == "b1024":
        return np.linspace(0., 0.7 * Lm, 1025)
    raise ValueError(kind)


def gram_edges(N, L):
    return kf(L) * np.array([0., 0.3, 1.5, 2.5, 0.3 * N, 0.5 * N, np.inf])      # (the first bin holds m_perp = 0 alone: empty)


# ---- the cases: shared by tests/test_binning_cases_cpu.py (which shows what each reaches) and tests/test_binning_exact_gpu.py ---
def power_edges_of(kind, N, L):
    if kind == "inside":                                               # first edge > 0 (a populated bin below), last inside the box
        return kf(L) * np.arange(2.5, 12.5)
    if kind == "coarse":
        return edges_coarse(N, L, 150)
    return {"between": edges_between, "narrow": edges_narrow, "on-shells": edges_on_shells}[kind](N, L)


# name: (N, L, edge set)
POWER_CASES = {"n16": (16, 100., "between"), "n18": (18, 100., "between"), "n24": (24, 100., "between"),
               "cuboid": (16, CUBOID, "between"), "narrow": (32, 100., "narrow"), "on-shells": (32, 100., "on-shells"),
               "inside": (32, 100., "inside")}
POWER_512 = (512, 100., "coarse")                                      # full layout, f32 only
WEDGE = ("wedge", 0.75, 0.25 * 2. * np.pi / 100.)
# name: (N, L, edge set, nmu, lmax, cross)
KMU_CASES = {"n16": (16, 100., "default", 5, 0, False), "n16-poles": (16, 100., "geometric", 3, 4, True),
             "n18": (18, 100., "default", 5, 0, True), "n18-poles": (18, 100., "uniform", 1, 4, False),
             "n24": (24, 100., "default", 5, 0, False), "n24-poles": (24, 100., "geometric", 3, 4, True),
             "cuboid": (16, CUBOID, "default", 5, 0, True), "cuboid-poles": (16, CUBOID, "uniform", 2, 4, False),
             "wide": (128, 100., "wide", 1, 0, False), "k40": (128, 100., "k40", 5, 0, True),
             "k1024x5": (32, 100., "k1024", 5, 0, False), "k1024-poles": (32, 100., "k1024", 1, 4, True),
             "k40x128": (32, 100., "k40", 128, 0, False),
             "uniform": (32, 100., "uniform", 4, 2, True), "geometric": (32, 100., "geometric", 4, 2, False),
             "early-done": (128, 100., "uniform", 2, 0, False)}
KMU_512 = (512, 100., "default", 1, 4, False)                          # half layout, f32 only
# name: (N, L, edge set, cross)
CYL_CASES = {"n16": (16, 100., "default", False), "n18": (18, 100., "default", True), "n24": (24, 100., "default", False),
             "cuboid": (16, CUBOID, "default", True), "one-row": (16, 100., "one-row", False),
             "ring32": (64, 100., "ring32", True), "tail": (64, 100., "tail", False), "n128": (128, 100., "default", True)}
CYL_512 = (512, 100., "default", False)
# name: (N, L, edge set, lmax)
SEP_CASES = {"n16": (16, 100., "all", 4), "n18": (18, 100., "all", 4), "n24": (24, 100., "all", 2),
             "cuboid": (16, CUBOID, "all", 4), "short": (32, 100., "short", 2), "wide": (128, 100., "wide", 0),
             "b1024": (32, 100., "b1024", 4)}
# (N, L)
CROSS_CASES = STANDARD + [(32, 100.)]
GRAM_CASES = [(16, 100.), (18, 100.), (24, 100.), (32, 100.), (64, 100.), (16, CUBOID)]
