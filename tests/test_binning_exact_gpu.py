"""GPU: the binning kernels alone, on the constructed integer inputs of tests/binning_cases.py (no FFT in the way), in both plan
precisions.  Every sum of integers must EQUAL the np.bincount reference bin by bin; the padding columns and the spare row of
every half-layout input hold NaN, so a kernel that reads them shows up as a NaN.  What each entry point is held to:

fb_bin_power, fb_bin_power_filtered (k_bin_rows, k_bin_count, k_bin_finish): count, sum |D|^2 and sum |D|^4 of every bin bit
    for bit, half and full layout, unfiltered, with the wedge mask and with a table of entries in {0, 0.5, 1, 2}.
fb_bin_power_kmu (k_pk_bin, k_bin_finish): modes per (k, mu) cell and sum P per cell (the integer sum times Lx Ly Lz / N^6,
    formed as bin_power_kmu forms it) bit for bit, auto and cross.  sum |k| and sum mu per cell within
    2^-53 (n_b + 8) sum_b w |x| of the extended-precision reference (x the summed quantity, n_b the stored modes of the cell).
    sum P L_l (l = 2, 4) per k bin within 2^-53 (n_b + 64) sum_b w |p| (times the same scale).
fb_bin_power_cyl (k_cyl_rows, k_cyl_finish): modes and sum P per (k_perp, k_par) cell bit for bit (the k = 0 mode excluded);
    sum k_perp and sum k_par within 2^-53 (n_b + 8) sum_b w |x|.
fb_bin_separation (k_sep_bin, k_bin_finish): cells per bin and sum xi per bin bit for bit (lmax = 0, and the l = 0 sums of
    every other call); sum |s| within 2^-53 (n_b + 8) sum_b |s|; sum xi L_l (l = 2, 4) within 2^-53 (n_b + 64) sum_b |xi|.
fb_cross_power_half (k_cross_power): every stored element bit-equal to conj(a) b scale (|a|^2 with imaginary part 0), k = 0
    exactly 0, out aliasing a or b the same bits, a sentinel in the padding columns and the spare row of out untouched.
fb_transverse_gram (k_maps_gram, k_maps_finish): modes per bin, and C bit-equal to the integer Gram sum times
    (Lx Ly / N^4) / modes_b formed as fb_cyl.hip forms it (NaN for an empty bin); the auto result exactly symmetric; sum k_perp
    within 2^-53 (n_b + 8) sum_b k_perp.
Every entry: a second call returns the same bytes, and no output is NaN where the reference is not.

The bounds.  A cell's device sum adds n_b terms in some order: at most n_b roundings, each below 2^-53 of a partial sum that
never exceeds sum_b |term|.  A term of sum |k| (mu, |s|) carries the roundings of the wavenumber itself: two or three squares,
two additions, a root, for mu a quotient -- below 8 units of 2^-53 relative.  A multipole term is w p L_l(mu^2) with mu^2 =
k_z^2 / k^2 as the kernels write it: k^2 carries at most 4 units relative (three products, two additions, all positive), the
square of k_z and the quotient one each: 6 units on mu^2 <= 1.  L_2 = 1.5 mu^2 - 0.5 turns them into 9, and adds 1.5 + 1 of its
own product and difference: 11.5 units absolute.  L_4 = ((35 mu^2 - 30) mu^2 + 3) / 8 has |dL_4 / d mu^2| <= 5: 30 units, and its
Horner steps round values of at most 35, 30, 30 and 8 before the exact division by 8: 13 units.  With the product by w p that is
at most about 45 units of 2^-53 per unit of w |p| (k_sep_bin forms mu = s_z / |s| and squares it: the same count within two
units), under the 64 allowed; the multiplication by the scale is one more.  Each bound is per cell, never relative to the largest
cell.  Largest measured ratio of error to bound over all cases (MI355X; each test prints its own):
    fb_bin_power_kmu    sum |k| 0.243, sum mu 0.248 (40 x 128 cells on 32^3: a few modes per cell), sum P L_2 0.007, sum P L_4 0.019
    fb_bin_power_cyl    sum k_perp 0.018, sum k_par below 0.0005
    fb_bin_separation   sum |s| 0.048, sum xi L_2 0.013, sum xi L_4 0.014
    fb_transverse_gram  sum k_perp below 0.0005

The two 512^3 inputs (a 1 GiB full and a 0.5 GiB half spectrum, single precision) are built once per module; their references
are formed x-plane by x-plane on the host, which is where their time goes.  Wall time on an MI355X host: the half spectrum built
and uploaded 0.5 s; test_bin_power_kmu_512 16.5 s (the extended-precision terms of four sums over 6.7e7 stored modes);
test_bin_power_cyl_512 0.9 s; test_bin_power_512_full 3.3 s with its own 1 GiB input.  Everything else is at most 128^3: the
other 110 tests take 5 s together."""
import time

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo, _lib
from fastbox_amd.device import FULL, HALF, REAL, DeviceArray
from tests import binning_cases as bc

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]
CD = {"f32": np.complex64, "f64": np.complex128}
RD = {"f32": np.float32, "f64": np.float64}
LD = np.longdouble
_BOXES = {}


def _box(N, L, prec):
    """(box, engine) of the case's geometry; the plan's layout is the one the cases file assumes."""
    key = (N, bc.sides(L), prec)
    if key not in _BOXES:
        if len(_BOXES) >= 4:
            _BOXES.clear()
        box = CosmoBox(cosmo=default_cosmo, box_scale=bc.box_scale(L), nsamp=N, realise_now=False, precision=prec)
        assert (box.Lx, box.Ly, box.Lz) == bc.sides(L)
        assert (N // 2 + 1, box.engine.rows, box.engine.pitch) == bc.half_dims(N)
        _BOXES[key] = box
    return _BOXES[key], _BOXES[key].engine


_REFS = {}


def _once(make, *key):
    """A reference is computed once and shared by the precisions (nothing writes to it)."""
    if key not in _REFS:
        _REFS[key] = make(*key)
    return _REFS[key]


def _pd(a):
    return a.ctypes.data_as(_lib.P_double)


def _ratio(dev, ref, bound):
    """max |dev - ref| / bound over the cells with a non-zero bound; where the bound is 0 the two must be equal."""
    err = np.abs(np.asarray(dev, dtype=LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    zero = bound == 0
    assert np.all(err[zero] == 0)
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.


# ---- fb_bin_power, fb_bin_power_filtered ---------------------------------------------------------------------------------------
def _bin_power(eng, spec, filt, table):
    if filt is None:
        return eng.bin_power(spec)
    if filt[0] == "wedge":
        return eng.bin_power(spec, (_lib.FB_FILT_WEDGE, (filt[1], filt[2], 0., 0.)))
    nb = eng._nbins
    out = [np.zeros(nb) for _ in range(3)]
    _lib.call("fb_bin_power_filtered", eng._plan, spec.ptr, 1 if spec.kind == HALF else 0, _lib.FB_FILT_TABLE, None, table.ptr,
              *[_pd(x) for x in out], eng.stream)
    return tuple(out)


def _check_bin_power(eng, N, L, e, layout, spec, filters, prec, label):
    eng.set_bins(e, *bc.shell_setup(N, L, e))
    for filt in filters:
        table = eng.upload_raw(bc.filter_table(N, layout, RD[prec])) if filt is not None and filt[0] == "table" else None
        got = _bin_power(eng, spec, filt, table)
        ref = _once(lambda *k: bc.ref_bin_power(N, L, e, layout, filt), "power", label, layout, filt)
        for name, g, r in zip(("count", "sum", "sumsq"), got, ref):
            assert not np.any(np.isnan(g)), (label, layout, filt, name)
            np.testing.assert_array_equal(g, r, err_msg="%s %s %s %s" % (label, layout, filt, name))
        again = _bin_power(eng, spec, filt, table)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    print("bin_power %s N=%d %s %s: %d bins, %d filters exact" % (label, N, prec, layout, e.size, len(filters)))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(bc.POWER_CASES))
def test_bin_power(name, prec):
    N, L, kind = bc.POWER_CASES[name]
    box, eng = _box(N, L, prec)
    e = bc.power_edges_of(kind, N, L)
    half = DeviceArray(eng, HALF, eng.upload_raw(bc.stored_half(N, 0, CD[prec])))
    full = DeviceArray(eng, FULL, eng.upload_raw(bc.stored_full(N, 0, CD[prec])))
    for layout, spec in (("half", half), ("full", full)):
        _check_bin_power(eng, N, L, e, layout, spec, (None, bc.WEDGE, ("table",)), prec, name)


# ---- fb_bin_power_kmu ----------------------------------------------------------------------------------------------------------
def _check_kmu(eng, N, L, kind, nmu, lmax, cross, h1, h2, label):
    e = np.ascontiguousarray(bc.kmu_edges(N, L, kind))
    nk = e.size - 1
    nc = nk * nmu
    out = np.full(4 * nc + (lmax // 2) * nk, -7.)
    args = (eng._plan, h1.ptr, h2.ptr if cross else None, _pd(e), nk, nmu, lmax)
    _lib.call("fb_bin_power_kmu", *args, _pd(out), eng.stream)
    ref = _once(lambda *k: bc.ref_kmu(N, L, e, nmu, lmax, cross), "kmu", N, bc.sides(L), kind, nmu, lmax, cross)
    assert not np.any(np.isnan(out)), label
    np.testing.assert_array_equal(out[:nc], ref["modes"], err_msg=label + " modes")
    scale = bc.power_scale(N, L)
    np.testing.assert_array_equal(out[3 * nc:4 * nc], ref["sum_int"] * scale, err_msg=label + " sum P")
    ratios = {}
    for key, at in (("sum_k", 1), ("sum_mu", 2)):
        ratios[key] = _ratio(out[at * nc:(at + 1) * nc], ref[key], bc.U * (ref["terms"] + 8.) * ref[key])
    for q, l in enumerate(range(2, lmax + 1, 2)):
        dev = out[4 * nc + q * nk:4 * nc + (q + 1) * nk]
        ratios["P L_%d" % l] = _ratio(dev, ref["poles"][l].astype(LD) * LD(scale),
                                      bc.U * (ref["terms_k"] + 64.) * ref["abs_k"] * scale)
    again = np.full_like(out, -7.)
    _lib.call("fb_bin_power_kmu", *args, _pd(again), eng.stream)
    assert again.tobytes() == out.tobytes(), label
    print("kmu %s N=%d nk=%d nmu=%d lmax=%d %s: modes and sum P exact; error / bound: %s"
          % (label, N, nk, nmu, lmax, "cross" if cross else "auto",
             ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    assert all(v <= 1. for v in ratios.values()), (label, ratios)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(bc.KMU_CASES))
def test_bin_power_kmu(name, prec):
    N, L, kind, nmu, lmax, cross = bc.KMU_CASES[name]
    box, eng = _box(N, L, prec)
    h1 = eng.upload_raw(bc.stored_half(N, 0, CD[prec]))
    h2 = eng.upload_raw(bc.stored_half(N, 1, CD[prec])) if cross else None
    _check_kmu(eng, N, L, kind, nmu, lmax, cross, h1, h2, "%s %s" % (name, prec))


# ---- fb_bin_power_cyl ----------------------------------------------------------------------------------------------------------
def _check_cyl(eng, N, L, kind, cross, h1, h2, label, wavenumbers=True):
    pe, qe = [np.ascontiguousarray(x) for x in bc.cyl_edges(N, L, kind)]
    nperp, npar = pe.size - 1, qe.size - 1
    nc = nperp * npar
    out = np.full(4 * nc, -7.)
    args = (eng._plan, h1.ptr, h2.ptr if cross else None, _pd(pe), nperp, _pd(qe), npar)
    _lib.call("fb_bin_power_cyl", *args, _pd(out), eng.stream)
    ref = _once(lambda *k: bc.ref_cyl(N, L, pe, qe, cross, wavenumbers), "cyl", N, bc.sides(L), kind, cross)
    assert not np.any(np.isnan(out)), label
    np.testing.assert_array_equal(out[:nc], ref["modes"], err_msg=label + " modes")
    np.testing.assert_array_equal(out[3 * nc:], ref["sum_int"] * bc.power_scale(N, L), err_msg=label + " sum P")
    ratios = {key: _ratio(out[at * nc:(at + 1) * nc], ref[key], bc.U * (ref["terms"] + 8.) * ref[key])
              for key, at in (("sum_kperp", 1), ("sum_kpar", 2)) if wavenumbers}
    again = np.full_like(out, -7.)
    _lib.call("fb_bin_power_cyl", *args, _pd(again), eng.stream)
    assert again.tobytes() == out.tobytes(), label
    print("cyl %s N=%d %d x %d cells %s: modes and sum P exact; error / bound: %s"
          % (label, N, nperp, npar, "cross" if cross else "auto", ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    assert all(v <= 1. for v in ratios.values()), (label, ratios)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(bc.CYL_CASES))
def test_bin_power_cyl(name, prec):
    N, L, kind, cross = bc.CYL_CASES[name]
    box, eng = _box(N, L, prec)
    h1 = eng.upload_raw(bc.stored_half(N, 0, CD[prec]))
    h2 = eng.upload_raw(bc.stored_half(N, 1, CD[prec])) if cross else None
    _check_cyl(eng, N, L, kind, cross, h1, h2, "%s %s" % (name, prec))


# ---- fb_bin_separation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(bc.SEP_CASES))
def test_bin_separation(name, prec):
    N, L, kind, lmax = bc.SEP_CASES[name]
    box, eng = _box(N, L, prec)
    e = np.ascontiguousarray(bc.sep_edges(N, L, kind))
    nb = e.size - 1
    xi = eng.upload(bc.real_field(N, 0, RD[prec]), REAL)
    ref = _once(lambda *k: bc.ref_separation(N, L, e, lmax), "sep", name)
    ratios = {}
    for lm in sorted({0, lmax}):
        out = np.full((2 + lm // 2 + 1) * nb, -7.)
        args = (eng._plan, xi.ptr, _pd(e), nb, lm)
        _lib.call("fb_bin_separation", *args, _pd(out), eng.stream)
        assert not np.any(np.isnan(out)), (name, lm)
        np.testing.assert_array_equal(out[:nb], ref["npairs"], err_msg="%s lmax=%d cells" % (name, lm))
        np.testing.assert_array_equal(out[2 * nb:3 * nb], ref["sum_int"], err_msg="%s lmax=%d sum xi" % (name, lm))
        ratios["sum_r"] = _ratio(out[nb:2 * nb], ref["sum_r"], bc.U * (ref["npairs"] + 8.) * ref["sum_r"])
        for q, l in enumerate(range(2, lm + 1, 2)):
            ratios["xi L_%d" % l] = _ratio(out[(3 + q) * nb:(4 + q) * nb], ref["poles"][l],
                                           bc.U * (ref["npairs"] + 64.) * ref["sum_abs"])
        again = np.full_like(out, -7.)
        _lib.call("fb_bin_separation", *args, _pd(again), eng.stream)
        assert again.tobytes() == out.tobytes(), (name, lm)
    print("separation %s N=%d %s nb=%d lmax=%d: cells and sum xi exact; error / bound: %s"
          % (name, N, prec, nb, lmax, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    assert all(v <= 1. for v in ratios.values()), (name, ratios)


# ---- fb_cross_power_half -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,L", bc.CROSS_CASES)
def test_cross_power_half(N, L, prec):
    box, eng = _box(N, L, prec)
    nzv, nr, nzp = bc.half_dims(N)
    a, b = bc.stored_half(N, 0, CD[prec]), bc.stored_half(N, 1, CD[prec])
    sentinel = CD[prec](complex(12345., -678.))
    scale = 2. ** -7

    def run(cross, alias):
        da, db = eng.upload_raw(a), eng.upload_raw(b)
        if alias is None:
            do = eng.upload_raw(np.full(a.shape, sentinel))
        else:
            do = da if alias == "a" else db
        _lib.call("fb_cross_power_half", eng._plan, da.ptr, db.ptr if cross else None, do.ptr, scale, eng.stream)
        return eng.download_raw(do, a.shape, CD[prec])

    for cross in (False, True):
        ref = bc.ref_cross_power(N, cross, scale, CD[prec])
        got = run(cross, None)
        np.testing.assert_array_equal(got[:, :N, :nzv], ref)
        assert got[0, 0, 0] == 0 and (cross or not np.any(got[:, :N, :nzv].imag))
        pad = np.full(a.shape, sentinel)
        assert got[:, N, :].tobytes() == pad[:, N, :].tobytes(), "the spare row of out was written"
        assert got[:, :, nzv:].tobytes() == pad[:, :, nzv:].tobytes(), "the padding columns of out were written"
        assert run(cross, None).tobytes() == got.tobytes()
        for alias, src in (("a", a), ("b", b)) if cross else (("a", a),):
            al = run(cross, alias)
            assert al[:, :N, :nzv].tobytes() == got[:, :N, :nzv].tobytes(), "out aliasing %s" % alias
            assert al[:, N, :].tobytes() == src[:, N, :].tobytes() and al[:, :, nzv:].tobytes() == src[:, :, nzv:].tobytes()
    print("cross_power N=%d %s: every element, k = 0, aliasing and the sentinel exact" % (N, prec))


# ---- fb_transverse_gram --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N,L", bc.GRAM_CASES)
def test_transverse_gram(N, L, cross, prec):
    box, eng = _box(N, L, prec)
    pe = np.ascontiguousarray(bc.gram_edges(N, L))
    nb = pe.size - 1
    f1 = eng.upload_raw(bc.stored_full(N, 0, CD[prec]))
    f2 = eng.upload_raw(bc.stored_full(N, 1, CD[prec])) if cross else None
    work = eng._alloc_bytes(_lib.load().fb_transverse_gram_work_bytes(eng._plan, nb, 1 if cross else 0))
    cl_dev = eng._alloc_bytes(nb * N * N * 8)
    modes, S, C, sumk = _once(lambda *k: bc.ref_gram(N, L, pe, cross), "gram", N, bc.sides(L), cross)

    def run():
        rec = np.full(2 * nb, -7.)
        _lib.call("fb_transverse_gram", eng._plan, f1.ptr, f2.ptr if cross else None, _pd(pe), nb, cl_dev.ptr, work.ptr,
                  _pd(rec), eng.stream)
        return rec, eng.download_raw(cl_dev, (nb, N, N))
    rec, cl = run()
    np.testing.assert_array_equal(rec[:nb], modes)
    empty = modes == 0
    assert np.array_equal(np.isnan(cl), np.isnan(C)) and np.all(np.isnan(cl[empty])) and not np.any(np.isnan(rec))
    assert cl[~empty].tobytes() == C[~empty].tobytes(), "C is not the integer Gram sum times (Lx Ly / N^4) / modes"
    if not cross:
        assert cl[~empty].tobytes() == np.ascontiguousarray(np.transpose(cl[~empty], (0, 2, 1))).tobytes()
    ratio = _ratio(rec[nb:], sumk, bc.U * (modes + 8.) * sumk)
    rec2, cl2 = run()
    assert rec2.tobytes() == rec.tobytes() and cl2.tobytes() == cl.tobytes()
    print("gram N=%d %s %s shape %s: modes and C exact; sum k_perp error / bound %.3f"
          % (N, prec, "cross" if cross else "auto", bc.gram_shape(N), ratio))
    assert ratio <= 1.


# ---- the two 512^3 inputs ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    _BOXES.clear()
    N, L = bc.KMU_512[:2]
    box = CosmoBox(cosmo=default_cosmo, box_scale=bc.box_scale(L), nsamp=N, realise_now=False, precision="f32")
    eng = box.engine
    assert (N // 2 + 1, eng.rows, eng.pitch) == bc.half_dims(N) and (box.Lx, box.Ly, box.Lz) == bc.sides(L)
    t0 = time.perf_counter()
    half = eng.upload_raw(bc.stored_half(N, 0, np.complex64))
    print("512^3 half spectrum built and uploaded in %.1f s" % (time.perf_counter() - t0))
    yield box, eng, half
    del half
    eng.release_idle_buffers()


def test_bin_power_kmu_512(big):
    box, eng, half = big
    N, L, kind, nmu, lmax, cross = bc.KMU_512
    t0 = time.perf_counter()
    _check_kmu(eng, N, L, kind, nmu, lmax, cross, half, None, "512 f32")
    print("kmu 512^3: %.1f s" % (time.perf_counter() - t0))


def test_bin_power_cyl_512(big):
    box, eng, half = big
    N, L, kind, cross = bc.CYL_512
    t0 = time.perf_counter()
    # (the two wavenumber sums are formed on the host by the library: checked at every other size, left out here)
    _check_cyl(eng, N, L, kind, cross, half, None, "512 f32", wavenumbers=False)
    print("cyl 512^3: %.1f s" % (time.perf_counter() - t0))


def test_bin_power_512_full(big):
    box, eng, half = big
    N, L, kind = bc.POWER_512
    t0 = time.perf_counter()
    full = DeviceArray(eng, FULL, eng.upload_raw(bc.stored_full(N, 0, np.complex64)))
    _check_bin_power(eng, N, L, bc.power_edges_of(kind, N, L), "full", full, (None,), "f32", "512")
    print("bin_power 512^3 full layout: %.1f s" % (time.perf_counter() - t0))
