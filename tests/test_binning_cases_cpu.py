"""CPU: the constructed binning cases (tests/binning_cases.py) are what they claim to be -- the patterns tell every stored mode of
a row apart and are not Hermitian, the poison lies where the kernels must not read, every sum stays below 2^53, the references
agree with the independent statements of tests/pk_numpy.py, cyl_numpy.py and corrfn_numpy.py -- and every case reaches the branch
it is in the table for, shown from the case alone with the launch decisions of the sources restated in the cases file."""
import numpy as np
import pytest

from tests import binning_cases as bc
from tests import corrfn_numpy as cf
from tests import cyl_numpy as cn
from tests import pk_numpy as pk


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_every_mode_of_a_row_is_distinguishable(which):
    for (i, j), nz in (((0, 0), 512), ((3, 5), 512), ((511, 510), 512), ((17, 2), 257)):
        re, im = [x[0, j] for x in bc.ints(512, nz, which, i)]
        assert np.max(np.abs(re)) <= 15 and np.max(np.abs(im)) <= 15
        assert np.unique(re * 100 + im).size == nz
    a, b = bc.ints(24, 24, 0, 0, 24), bc.ints(24, 24, 1, 0, 24)
    assert np.any(a[0] != b[0]) and np.any(a[1] != b[1])
    # neighbouring rows and planes differ in every element: a row read in place of the next one changes the sums
    v = a[0] * 100 + a[1]
    assert np.all(v[:, 1:] != v[:, :-1]) and np.all(v[1:] != v[:-1])


def test_spectra_are_not_hermitian_and_fields_are_small_integers():
    N = 16
    f = bc.stored_full(N, 0, np.complex128)
    idx = (-np.arange(N)) % N
    assert not np.array_equal(f, np.conj(f[np.ix_(idx, idx, idx)]))
    r = bc.real_field(N, 0, np.float32)
    assert r.dtype == np.float32 and np.array_equal(r, np.rint(r)) and np.abs(r).max() == 15
    t = bc.filter_table(N, "full", np.float32)
    assert set(np.unique(t)) == {0., 0.5, 1., 2.}


@pytest.mark.parametrize("N", [16, 18, 24, 32, 128])
@pytest.mark.parametrize("cdtype", [np.complex64, np.complex128])
def test_half_layout_and_poison(N, cdtype):
    nzv, nr, nzp = bc.half_dims(N)
    assert (nzv, nr) == (N // 2 + 1, N + 1) and nzp % 16 == 0 and nzv <= nzp < nzv + 16
    h = bc.stored_half(N, 0, cdtype)
    assert h.shape == (N, nr, nzp) and h.dtype == cdtype and h.flags.c_contiguous
    assert np.all(np.isnan(h[:, N, :].real)) and np.all(np.isnan(h[:, N, :].imag))
    assert np.all(np.isnan(h[:, :, nzv:].real)) and np.all(np.isnan(h[:, :, nzv:].imag))
    re, im = bc.ints(N, nzv, 0, 0, N)
    assert np.array_equal(h[:, :N, :nzv].real, re) and np.array_equal(h[:, :N, :nzv].imag, im)
    t = bc.filter_table(N, "half", np.float32)
    assert np.all(np.isnan(t[:, N, :])) and np.all(np.isnan(t[:, :, nzv:])) and not np.any(np.isnan(t[:, :N, :nzv]))
    if N == 18:
        assert N % 4 == 2 and nzv == 10


def test_every_sum_stays_exact():
    """|D|^2 <= 450 needs 9 bits (exact in fp32, times a table entry squared 13); the largest sum any case can form is
    sum 2 |D|^4 over 512^3 modes < 2^46.  The references assert the same of the sums they form."""
    assert 2 * 15 ** 2 == 450 and 450 < 2 ** 24 and 4 * 450 * 4 < 2 ** 24
    assert 2 * 450 ** 2 * 512 ** 3 < 2 ** 46 < bc.EXACT
    assert 2 * 15 * 15 * 1024 ** 2 < bc.EXACT                          # a Gram sum over every transverse mode


def test_cellsums_adds_extended_terms_exactly():
    ld = np.longdouble
    t = np.array([ld(1), ld(2) ** -60, -ld(1), ld(2) ** -60, ld(3)], dtype=ld)
    s = bc.CellSums(3)
    s.add(np.array([0, 0, 0, 0, 2]), t)
    assert np.array_equal(s.result(), [2. ** -59, 0., 3.])
    s = bc.CellSums(2, limit=2)                                        # flushed in pieces: each piece's sum is rounded once
    for c, v in zip([0, 1, 0, 0], [1e16, 5., 1., -1e16]):
        s.add(np.array([c]), np.array([v], dtype=ld))
    r = s.result()
    assert abs(r[0] - 1.) <= bc.U * 2e16 and r[1] == 5.
    s = bc.CellSums(2)                                                 # in one batch: exact
    s.add(np.array([0, 1, 0, 0]), np.array([1e16, 5., 1., -1e16], dtype=ld))
    assert np.array_equal(s.result(), [1., 5.])


# ---- references against independent statements -------------------------------------------------------------------------------
def test_shell_binning_is_digitize_of_the_exact_wavenumber():
    """On a cube whose size has no rounding quirk the thresholds restate np.digitize(|k|, edges) of every mode."""
    for name in ("n16", "inside", "narrow"):
        N, L, kind = bc.POWER_CASES[name]
        e = bc.power_edges_of(kind, N, L)
        thr, amb = bc.shell_setup(N, L, e)
        assert thr is not None and len(amb) == 0
        for layout, nz in (("full", N), ("half", N // 2 + 1)):
            assert np.array_equal(bc.power_bins(N, L, e, layout, 0, N), np.digitize(bc.kmag_planes(N, L, nz, 0, N), e))


@pytest.mark.parametrize("name", ["n16", "n18", "cuboid", "on-shells"])
def test_power_reference(name):
    N, L, kind = bc.POWER_CASES[name]
    e = bc.power_edges_of(kind, N, L)
    ch, sh, qh = bc.ref_bin_power(N, L, e, "half")
    cf_, sf, qf = bc.ref_bin_power(N, L, e, "full")
    assert np.array_equal(ch, cf_) and ch.sum() <= N ** 3 and not np.array_equal(sh, sf)     # (not Hermitian)
    # by loops over the stored modes
    f = bc.stored_full(N, 0, np.complex128)
    b = bc.power_bins(N, L, e, "full", 0, N)
    want = np.zeros((2, e.size + 1))
    for idx in np.ndindex(N, N, N):
        p = int(f[idx].real) ** 2 + int(f[idx].imag) ** 2
        want[0, b[idx]] += p
        want[1, b[idx]] += p * p
    assert np.array_equal(sf, want[0, :-1]) and np.array_equal(qf, want[1, :-1])
    # filters: the mask keeps integers, the table's entries are dyadic
    for filt in (bc.WEDGE, ("table",)):
        c, s, q = bc.ref_bin_power(N, L, e, "half", filt)
        assert np.array_equal(c, ch) and np.all(s <= sh * 4) and np.array_equal(s * 4, np.rint(s * 4)) and s.sum() > 0
        assert not np.array_equal(s, sh)
    t = bc.filter_multiplier(N, L, "half", bc.WEDGE, 0, N)
    assert 0.1 < t.mean() < 0.9


@pytest.mark.parametrize("name", ["n16-poles", "cuboid-poles", "n18"])
def test_kmu_reference(name):
    N, L, kind, nmu, lmax, cross = bc.KMU_CASES[name]
    e = bc.kmu_edges(N, L, kind)
    r = bc.ref_kmu(N, L, e, nmu, lmax, cross)
    s = pk.power_sums(np.zeros((N, N, N)), None, bc.sides(L), e, Nmu=nmu, lmax=0)
    assert np.array_equal(r["modes"], s["modes"].ravel()) and r["modes"].sum() > N ** 3 // 4
    for a, b in ((r["sum_k"], s["sum_k"]), (r["sum_mu"], s["sum_mu"])):
        assert np.all(np.abs(a - b.ravel()) <= 1e-13 * np.abs(a))
    # the integer sums and the multipoles by the double-precision statement on the same stored values
    nz = N // 2 + 1
    h1 = bc.stored_half(N, 0, np.complex128)[:, :N, :nz]
    h2 = bc.stored_half(N, 1, np.complex128)[:, :N, :nz] if cross else h1
    P = (np.conj(h1) * h2).real
    kx, ky, kz = pk.wavenumbers(N, bc.sides(L))
    K = np.sqrt((kx[:, None, None] ** 2 + ky[None, :, None] ** 2) + kz[None, None, :nz] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(K > 0, np.abs(kz[None, None, :nz]) / K, 0.)
    cell, ok = pk._bin_cells(K, mu, e, nmu)
    w = bc.mode_weight(N, "half")[None, None, :] * np.ones_like(K)
    assert np.array_equal(r["sum_int"], np.bincount(cell[ok], weights=(w * P)[ok], minlength=r["modes"].size))
    for l, v in r["poles"].items():
        d = np.bincount(cell[ok] // nmu, weights=(w * P * pk.legendre(l, mu))[ok], minlength=e.size - 1)
        assert np.all(np.abs(v - d) <= 1e-12 * r["abs_k"]) and np.any(v != 0)


@pytest.mark.parametrize("name", ["n16", "cuboid", "one-row"])
def test_cyl_reference(name):
    N, L, kind, cross = bc.CYL_CASES[name]
    pe, qe = bc.cyl_edges(N, L, kind)
    r = bc.ref_cyl(N, L, pe, qe, cross)
    s = cn.cyl_sums(np.zeros((N, N, N)), None, bc.sides(L), pe, qe)
    assert np.array_equal(r["modes"], s["modes"].ravel())
    for a, b in ((r["sum_kperp"], s["sum_kperp"]), (r["sum_kpar"], s["sum_kpar"])):
        assert np.all(np.abs(a - b.ravel()) <= 1e-13 * np.abs(a))
    assert np.any(r["sum_int"] != 0) and np.all(np.abs(r["sum_int"]) <= r["sum_abs"])


@pytest.mark.parametrize("name", ["n16", "cuboid", "short"])
def test_separation_reference(name):
    N, L, kind, lmax = bc.SEP_CASES[name]
    e = bc.sep_edges(N, L, kind)
    r = bc.ref_separation(N, L, e, lmax)
    poles = list(range(0, lmax + 1, 2))
    rr, xil, npairs = cf.bin_xi(bc.real_field(N, 0, np.float64), bc.sides(L), e, poles)
    assert np.array_equal(npairs, r["npairs"]) and npairs.sum() > 0
    m = npairs > 0
    assert np.all(np.abs((xil[0] * npairs)[m] - r["sum_int"][m]) <= 1e-13 * r["sum_abs"][m]) and np.any(r["sum_int"] != 0)
    assert np.all(np.abs(rr[m] * npairs[m] - r["sum_r"][m]) <= 1e-13 * r["sum_r"][m])
    for q, l in enumerate(poles[1:], 1):
        assert np.all(np.abs(xil[q][m] * npairs[m] / (2 * l + 1) - r["poles"][l][m]) <= 1e-12 * r["sum_abs"][m])


@pytest.mark.parametrize("cross", [False, True])
def test_gram_and_cross_power_references(cross):
    N, L = 16, bc.CUBOID
    pe = bc.gram_edges(N, L)
    modes, S, C, sk = bc.ref_gram(N, L, pe, cross)
    a1 = bc.stored_full(N, 0, np.complex128).reshape(N * N, N)
    a2 = bc.stored_full(N, 1, np.complex128).reshape(N * N, N) if cross else a1
    kp = cn.kperp_plane(N, L).ravel()
    b, ok = cn._digitize(kp, pe)
    ok[0] = False
    for q in range(pe.size - 1):
        sel = ok & (b == q)
        assert modes[q] == np.count_nonzero(sel)
        assert np.array_equal(S[q], np.einsum("mi,mj->ij", a1[sel], np.conj(a2[sel])).real)
        if modes[q]:
            assert np.allclose(C[q], S[q] * L[0] * L[1] / N ** 4 / modes[q], rtol=1e-15, atol=0)
            assert abs(sk[q] - kp[sel].sum()) <= 1e-13 * sk[q]
        else:
            assert np.all(np.isnan(C[q]))
    assert (modes == 0).any() and modes.sum() == N * N - 1
    if not cross:
        assert np.array_equal(S, np.transpose(S, (0, 2, 1)))
    else:
        assert not np.array_equal(S, np.transpose(S, (0, 2, 1)))
    nz = N // 2 + 1
    h1 = bc.stored_half(N, 0, np.complex128)[:, :N, :nz]
    h2 = bc.stored_half(N, 1, np.complex128)[:, :N, :nz]
    for cdtype in (np.complex64, np.complex128):
        x = bc.ref_cross_power(N, cross, 2. ** -7, cdtype)
        want = (np.conj(h1) * (h2 if cross else h1)) * 2. ** -7
        want[0, 0, 0] = 0
        assert x.dtype == cdtype and np.array_equal(x, want)
        assert cross or not np.any(x.imag)


# ---- every case reaches its branch -------------------------------------------------------------------------------------------
def test_general_cases():
    (n16, l16), (n18, _), (n24, _), (nc, lc) = bc.STANDARD
    assert n16 == 16 and bc.half_dims(16)[0] == 9 < 64                 # one step per row, every lane group partly past the end
    assert n18 % 4 == 2 and bc.half_dims(18)[0] == 10
    assert n24 & (n24 - 1) and n18 & (n18 - 1)                         # two sizes that are no power of two
    assert len(set(bc.sides(lc))) == 3 and bc.shell_setup(nc, lc, bc.edges_between(nc, lc))[0] is None
    for name in ("n16", "n18", "n24"):
        N, L, kind = bc.POWER_CASES[name]
        thr, amb = bc.shell_setup(N, L, bc.power_edges_of(kind, N, L))
        assert thr is not None and bc.bin_rows_steps(N, "full") == 1


def test_bin_rows_cases():
    N, L, kind = bc.POWER_CASES["narrow"]
    e = bc.power_edges_of(kind, N, L)
    assert e.size == 200 and bc.shell_setup(N, L, e)[0] is not None
    span, _, _ = bc.bin_rows_spans(N, L, e)
    assert span.min() > bc.BIN_MAXSPAN                                 # every row takes the wave_flush path ...
    n, l, k = bc.POWER_CASES["n16"]                                    # ... none of these: the wave-sum path ...
    assert bc.bin_rows_spans(n, l, bc.power_edges_of(k, n, l))[0].max() <= bc.BIN_MAXSPAN
    for other in ("n24", "inside"):                                    # ... and these have rows of both kinds
        n, l, k = bc.POWER_CASES[other]
        sp = bc.bin_rows_spans(n, l, bc.power_edges_of(k, n, l))[0]
        assert sp.min() <= bc.BIN_MAXSPAN < sp.max()
    N, L, kind = bc.POWER_CASES["on-shells"]
    e = bc.power_edges_of(kind, N, L)
    thr, amb = bc.shell_setup(N, L, e)
    assert thr is not None and 1 <= len(amb) <= 8
    m = pk.signed_index(N)
    n2 = m[:, None, None] ** 2 + m[None, :, None] ** 2 + m[None, None, :] ** 2
    assert all(np.any(n2 == a) for a in amb)
    N, L, kind = bc.POWER_CASES["inside"]
    e = bc.power_edges_of(kind, N, L)
    b = bc.power_bins(N, L, e, "half", 0, N)
    assert e[0] > 0 and np.count_nonzero(b == 0) > 30 and np.count_nonzero(b == e.size) > 100
    assert set(np.unique(b)) == set(range(e.size + 1))
    N, L, kind = bc.POWER_512
    assert N == 512 > 64 * bc.BIN_GROUP and bc.bin_rows_steps(N, "full") == 2 and bc.bin_rows_steps(N, "half") == 1
    assert all(bc.bin_rows_steps(n, "full") == 1 for n in (16, 18, 24, 32, 64, 128, 256, 320))
    assert bc.power_edges_of(kind, N, L).size <= 256


def _first_step_keys(N, L, e, nmu):
    return [bc.pk_row_keys(N, L, e, nmu, i, j)[0][:64] for i in (0, 1, 5, N // 2) for j in (0, 2, N - 3)]


def test_pk_bin_cases():
    # one wide bin: a 64-lane step inside one cell, and a second step with one live lane
    N, L, kind, nmu, lmax, cross = bc.KMU_CASES["wide"]
    e = bc.kmu_edges(N, L, kind)
    assert (e.size - 1, nmu) == (1, 1) and bc.half_dims(N)[0] == 65
    keys = bc.pk_row_keys(N, L, e, nmu, 3, 4)[0]
    assert np.all(keys[:64] == 0) and keys[64] == 0
    assert bc.pk_row_keys(N, L, e, nmu, 0, 0)[0][0] == -1              # k = 0
    # 40 x 5 cells: many runs in one step
    N, L, kind, nmu, lmax, cross = bc.KMU_CASES["k40"]
    e = bc.kmu_edges(N, L, kind)
    assert (e.size - 1, nmu) == (40, 5)
    runs = [np.count_nonzero(np.diff(k)) + 1 for k in _first_step_keys(N, L, e, nmu)]
    assert max(runs) >= 32 and all(np.all(np.diff(k) >= 0) for k in _first_step_keys(N, L, e, nmu))
    # the largest layouts
    shapes = []
    for name in ("k1024x5", "k1024-poles", "k40x128"):
        N, L, kind, nmu, lmax, cross = bc.KMU_CASES[name]
        nk, nv = bc.kmu_edges(N, L, kind).size - 1, lmax // 2 + 1
        waves = bc.pk_waves(nk, nmu, nv)
        shapes.append((nk, nmu, lmax, waves, nk * nmu * nv))
        assert bc.pk_lds(nk, nmu, nv, waves) > bc.LDS_DEFAULT and bc.pk_lds(nk, nmu, nv, waves) <= bc.LDS_CU
    assert shapes == [(1024, 5, 0, 3, 5120), (1024, 1, 4, 4, 3072), (40, 128, 0, 3, 5120)]
    # both bin guesses; key -1; rows beyond the last edge
    for name, uni in (("uniform", True), ("geometric", False)):
        N, L, kind, nmu, lmax, cross = bc.KMU_CASES[name]
        e = bc.kmu_edges(N, L, kind)
        assert bc.pk_uniform(e) is uni and e[0] > 0
        kperp = bc.pk_kperp(N, L)
        assert np.any(kperp >= e[-1]) and np.any(kperp < e[-1])
        keys = np.array([bc.pk_row_keys(N, L, e, nmu, i, j)[0] for i in range(N) for j in range(N)])
        assert np.count_nonzero(keys == -1) > 1 and np.any(keys == 1 << 30) and np.any((keys >= 0) & (keys < 1 << 30))
    assert bc.pk_uniform(bc.kmu_edges(16, 100., "default")) and not bc.pk_uniform(bc.kmu_edges(128, 100., "wide"))
    # a row that ends early: its second step starts beyond the last edge
    N, L, kind, nmu, lmax, cross = bc.KMU_CASES["early-done"]
    e = bc.kmu_edges(N, L, kind)
    K = bc.pk_row_keys(N, L, e, nmu, 1, 2)[1]
    assert K[0] < e[-1] <= K[64] and bc.half_dims(N)[0] > 64
    # 512: a second group of loads
    N, L, kind, nmu, lmax, cross = bc.KMU_512
    assert bc.half_dims(N)[0] == 257 > 64 * bc.PK_GROUP and lmax == 4 and bc.kmu_edges(N, L, kind).size - 1 == 256


def test_cyl_cases():
    N, L, kind, cross = bc.CYL_CASES["one-row"]
    pe, qe = bc.cyl_edges(N, L, kind)
    rc, rows, lengths = bc.cyl_chunks(N, L, pe)
    assert rows[0] == 1 and rows[2] == 0 and np.all(rows[[1, 3, 4, 5]] > 0)
    r = bc.ref_cyl(N, L, pe, qe, cross)["modes"].reshape(pe.size - 1, qe.size - 1)
    assert r[0, 0] == 0 and r[0, 1] == 4 and np.all(r[:, 2] == 0)      # [0, 0.5 k_f) x [0, 0.5 k_f) holds k = 0 alone: excluded
    seen4, seen16, several = set(), set(), False
    for name in ("ring32", "tail"):
        N, L, kind, cross = bc.CYL_CASES[name]
        rc, rows, lengths = bc.cyl_chunks(N, L, bc.cyl_edges(N, L, kind)[0])
        assert (N, rc) == (64, 32)
        several |= bool(np.any(rows > 3 * rc))
        seen4 |= {n % 4 for n in lengths}
        seen16 |= {n % 16 for n in lengths}
    assert several and {1, 2, 3} <= seen4 and {1, 2, 3} <= seen16
    N = bc.CYL_CASES["n128"][0]
    assert bc.half_dims(N)[0] == 65                                    # two m_z tiles of 64, the second with one live lane
    assert bc.CYL_512[:2] == bc.KMU_512[:2]                            # the 512^3 input of k_pk_bin again
    pe, qe = bc.cyl_edges(*bc.CYL_512[:3])
    assert pe.size - 1 <= 1024 and qe.size - 1 <= 1025


def test_sep_cases():
    for name in ("n16", "n18"):
        N, L, kind, lmax = bc.SEP_CASES[name]
        e = bc.sep_edges(N, L, kind)
        assert e[-1] >= np.sqrt(3.) / 2. * L and bc.sep_reach(N, L, e[-1]) == [N // 2] * 3
        r = bc.ref_separation(N, L, e, 0)
        assert r["npairs"].sum() == N ** 3                             # every cell visited, the lines at 0 and N/2 included
    N, L, kind, lmax = bc.SEP_CASES["short"]
    e = bc.sep_edges(N, L, kind)
    assert e[-1] == L / 8. and all(m < N // 2 for m in bc.sep_reach(N, L, e[-1]))
    M = bc.sep_reach(N, L, e[-1])[0]
    assert bc.sep_row_bins(N, L, e, M, M)[0] >= e.size - 1             # a visited row that lies beyond the last edge
    assert np.any(bc.sep_row_bins(N, L, e, 0, 0) < 0)                  # cells below the first edge
    N, L, kind, lmax = bc.SEP_CASES["wide"]
    e = bc.sep_edges(N, L, kind)
    b = bc.sep_row_bins(N, L, e, 3, 4)
    assert e.size == 2 and np.all(b[:64] == 0) and b.size == 65        # a whole step in one bin, then one live lane
    N, L, kind, lmax = bc.SEP_CASES["b1024"]
    e = bc.sep_edges(N, L, kind)
    assert e.size - 1 == 1024 and lmax == 4 and bc.LDS_DEFAULT < bc.sep_lds(1024, 3) <= bc.LDS_CU
    assert bc.sep_lds(1024, 2) > bc.LDS_DEFAULT                        # the geometry pass, too


def test_gram_cases():
    shapes = {N: bc.gram_shape(N) for N, L in bc.GRAM_CASES if bc.sides(L)[0] == bc.sides(L)[2]}
    assert shapes[16] == (1, False) and shapes[24] == (1, True) and shapes[32] == (2, False) and shapes[64] == (4, False)
    assert shapes[18] == (1, True)
    for N, L in bc.GRAM_CASES:
        for cross in (False, True):
            for num_cu in (64, 104, 228, 256, 304):                    # (the chunk length depends on the device: 256 on an MI355X)
                rc = bc.gram_chunk_rows(N, N * N - 1, cross, num_cu)
                assert rc == 16                                        # grids this small: the floor of 16 modes on every device
                rc, rows, lengths = bc.cyl_chunks(N, L, bc.gram_edges(N, L), skip0=True, rc=rc)
                assert rows.sum() == N * N - 1 and (rows == 0).any()
                assert any(n % 4 for n in lengths)                     # a masked last rank-4 update
    assert bc.gram_chunk_rows(1024, 1024 ** 2 - 1, False, 8) > 16      # (the formula, away from its floor)
