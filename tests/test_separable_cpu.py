"""CPU: the separable reference of tests/separable_numpy.py against numpy's own N^3 transforms at sizes where those are cheap,
the exactness of every case in float32 storage, the yardstick of the rms bounds, and the sensitivity of the comparison the
GPU tests make (tests/test_large_grid_reference_gpu.py): without this file a wrong helper would silently define what "correct"
means there."""
import numpy as np
import pytest

from tests import separable_numpy as sn

SIZES = [16, 24, 32]


def _rms(a):
    return np.sqrt(np.mean(np.abs(a) ** 2))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name", sn.CASES)
def test_separable_reference_equals_numpy(name, N):
    terms = sn.case_terms(name, N)
    x = sn.field(terms)
    f = sn.factor_spectra(terms)
    want = np.fft.fftn(x)
    got = sn.spectrum(f)
    assert np.max(np.abs(got - want)) <= 1e-13 * _rms(want), (name, N, np.max(np.abs(got - want)) / _rms(want))
    half = sn.spectrum(f, N // 2 + 1)
    ref = np.fft.rfftn(x)
    assert np.max(np.abs(half - ref)) <= 1e-13 * _rms(ref)
    # the inverse of a real field's transform factor by factor: ifftn(x) = conj(fftn(x)) / N^3
    inv = np.fft.ifftn(x)
    assert np.max(np.abs(np.conj(got) / N ** 3 - inv)) <= 1e-13 * _rms(inv)
    # and the field back from its half spectrum (what the c2r tests compare with)
    back = np.fft.irfftn(half, s=(N, N, N), axes=(0, 1, 2))
    assert np.max(np.abs(back - x)) <= 1e-13 * max(_rms(x), np.max(np.abs(x)) / N ** 1.5)


@pytest.mark.parametrize("N", SIZES)
def test_complex_inputs_are_the_same_combination(N):
    for p, q in sn.complex_pairs():
        tp, tq = sn.case_terms(p, N), sn.case_terms(q, N)
        x = sn.field(tp) + 1j * sn.field(tq)
        fp, fq = sn.spectrum(sn.factor_spectra(tp)), sn.spectrum(sn.factor_spectra(tq))
        want = np.fft.fftn(x)
        assert np.max(np.abs(fp + 1j * fq - want)) <= 1e-13 * _rms(want), (p, q)
        inv = np.fft.ifftn(x)
        assert np.max(np.abs((np.conj(fp) + 1j * np.conj(fq)) / N ** 3 - inv)) <= 1e-13 * _rms(inv), (p, q)
        assert np.array_equal(x.astype(np.complex64).astype(np.complex128), x)
    names = [p for p, _ in sn.complex_pairs()] + [q for _, q in sn.complex_pairs()]
    assert sorted(names) == sorted(2 * list(sn.CASES))


@pytest.mark.parametrize("N", SIZES + [512, 2048])
@pytest.mark.parametrize("name", sn.CASES)
def test_every_case_is_exact_in_float32(name, N):
    terms = sn.case_terms(name, N)
    for t in terms:
        for v in t:
            assert np.array_equal(np.rint(v * 128.), v * 128.) and np.max(np.abs(v)) <= 1.0       # 8 significant bits
    planes = range(N) if N <= 32 else (0, 1, 2, N // 2, N - 1)
    for i in planes:
        p = sn.field_plane(terms, i)
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p), (name, N, i)
    if N <= 32:
        # the planes are what the device builds: products and sums in fp64, then one cast -- no rounding anywhere
        x = sn.field(terms)
        scaled = x * 2.0 ** 21
        assert np.array_equal(np.rint(scaled), scaled) and np.max(np.abs(x)) < 4.0


def test_case_list():
    N = 32
    H = N // 2
    x = sn.field(sn.case_terms("impulse_a", N))
    assert x[1, N - 1, H + 1] == 1.0 and np.sum(np.abs(x)) == 1.0
    x = sn.field(sn.case_terms("impulse_b", N))
    assert x[N - 1, H, 1] == 1.0 and np.sum(np.abs(x)) == 1.0
    x = sn.field(sn.case_terms("impulse_origin", N))
    assert x[0, 0, 0] == 1.0 and np.sum(np.abs(x)) == 1.0
    i = np.arange(N)
    assert np.array_equal(sn.field(sn.case_terms("nyquist", N)), (-1.0) ** (i[:, None, None] + i[None, :, None] + i[None, None, :]))
    two = sn.case_terms("two_term", N)
    assert np.all(two[0][0][1::2] == 0) and np.all(two[1][0][0::2] == 0)
    assert np.linalg.matrix_rank(sn.field(two).reshape(N, N * N)) == 2                              # no longer rank 1
    # the single mode: its transform peaks at (m, N - m, N/2 - 1) and the mirror image, the rest is the 8-bit rounding
    m = sn.single_mode_index(N)
    F = np.abs(np.fft.fftn(sn.field(sn.case_terms("single_mode", N))))
    assert np.unravel_index(np.argmax(F[:, :, :H]), (N, N, H)) == m and F[m] > 0.49 * N ** 3
    F[m] = F[tuple((-k) % N for k in m)] = 0.0
    assert F.max() < 0.01 * N ** 3
    # the transform of an impulse has modulus 1 everywhere
    for name in ("impulse_origin", "impulse_a", "impulse_b"):
        assert np.max(np.abs(np.abs(sn.spectrum(sn.factor_spectra(sn.case_terms(name, N)))) - 1.0)) < 1e-14


def test_yardstick_of_the_rms_bounds():
    """scipy's single- and double-precision transforms at 256^3 against a higher precision: the numbers the GPU tests scale."""
    r32, m32 = sn.yardstick("f32")
    r64, m64 = sn.yardstick("f64")
    print("yardstick 256^3: f32 rms %.3e max %.3e   f64 rms %.3e max %.3e" % (r32, m32, r64, m64))
    # a few unit roundoffs per element, growing like the square root of the levels: anything else is not a yardstick
    assert 0.5 * sn.EPS["f32"] < r32 < 10 * sn.EPS["f32"] and m32 < 20 * r32
    assert 0.5 * sn.EPS["f64"] < r64 < 10 * sn.EPS["f64"] and m64 < 20 * r64
    assert sn.rms_bound("f32", 2048) == 3.0 * r32 * np.sqrt(33.0 / 24.0)


def _stand_in(x, precision):
    """an independent transform in the precision of the plan under test (scipy's), in the role of the kernel"""
    import scipy.fft
    if precision == "f32":
        out = scipy.fft.fftn(x.astype(np.float32))
        assert out.dtype == np.complex64
        return out.astype(np.complex128)
    return scipy.fft.fftn(x)


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", sn.CASES)
def test_the_comparison_can_fail(name, precision):
    """The check the GPU tests apply passes on a correct transform of the right precision and fails when ONE mode is
    conjugated, or when two modes of one |k| shell are swapped -- errors that leave the sum of squares, Parseval and a
    shell-binned P(k) unchanged."""
    N = 32
    terms = sn.case_terms(name, N)
    want = sn.spectrum(sn.factor_spectra(terms))
    got = _stand_in(sn.field(terms), precision)
    sn.check(got, want, precision, name)
    # the mode with the largest imaginary part, and the mode of its |k| shell that differs most from it.  Two spectra are
    # real and constant on shells by nature -- the impulse at the origin (all ones) and the Nyquist wave (one real mode) --
    # so these two perturbations are the identity on them; every other case must notice both
    m = np.minimum(np.arange(N), N - np.arange(N)) ** 2
    n2 = m[:, None, None] + m[None, :, None] + m[None, None, :]
    a = np.unravel_index(np.argmax(np.abs(want.imag)), want.shape)
    same = np.where(n2 == n2[a], np.abs(want - want[a]), -1.0)
    b = np.unravel_index(np.argmax(same), want.shape)
    degenerate = name in ("impulse_origin", "nyquist")
    assert (abs(want[a].imag) < 1e-9 and abs(want[a] - want[b]) < 1e-9) == degenerate, name
    if degenerate:
        # what these two can show instead: the Nyquist wave's one mode landing on a neighbouring mode, and (every permutation
        # and conjugation being the identity on a spectrum of ones) a twiddle of the impulse off by a phase of 1e-4 rad (f32)
        # / 1e-12 rad (f64)
        bad = got.copy()
        if name == "nyquist":
            pk = np.unravel_index(np.argmax(np.abs(want)), want.shape)
            nb = (pk[0], pk[1], pk[2] - 1)
            bad[pk], bad[nb] = got[nb], got[pk]
        else:
            bad[3, 2, 1] *= np.exp(1j * (1e-4 if precision == "f32" else 1e-12))
        with pytest.raises(AssertionError):
            sn.check(bad, want, precision, name)
        return
    conj = got.copy()
    conj[a] = np.conj(conj[a])
    with pytest.raises(AssertionError):
        sn.check(conj, want, precision, name)
    swap = got.copy()
    swap[a], swap[b] = got[b], got[a]
    with pytest.raises(AssertionError):
        sn.check(swap, want, precision, name)
    assert np.isclose(np.sum(np.abs(conj) ** 2), np.sum(np.abs(got) ** 2), rtol=1e-12)
    assert np.isclose(np.sum(np.abs(swap) ** 2), np.sum(np.abs(got) ** 2), rtol=1e-12)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_the_chunked_device_comparison_can_fail(precision):
    """The form the GPU tests run -- _Rig.fill / compare / _judge of tests/test_large_grid_reference_gpu.py, chunk by chunk in
    torch -- here on the CPU at 32^3 with scipy's transform in the role of the kernel: clean on the correct output, a
    finding when one mode is conjugated or two modes of one shell are swapped."""
    import torch
    from tests import test_large_grid_reference_gpu as lg
    N = 32
    rig = object.__new__(lg._Rig)
    rig.torch, rig.N, rig.H, rig.nz, rig.precision, rig.dev = torch, N, N // 2, N // 2 + 1, precision, torch.device("cpu")
    rig.rdtype = torch.float32 if precision == "f32" else torch.float64
    rig.chunks = lambda nlast: [(i, i + 5 if i + 5 < N else N) for i in range(0, N, 5)]           # ragged chunks
    for name in ("random", "two_term", "impulse_a", "single_mode", "mixed"):
        terms = sn.case_terms(name, N)
        x = torch.empty((N, N, N), dtype=rig.rdtype)
        rig.fill(x, rig.factors(terms), N)
        assert np.array_equal(x.numpy().astype(np.float64), sn.field(terms))
        good = torch.from_numpy(_stand_in(x.numpy().astype(np.float64), precision)[:, :, :rig.nz].copy())
        spec = rig.spectra(terms)
        log, fails = [], []
        lg._judge(rig, name, [name], rig.compare(good, [(1, spec)], rig.nz), log, fails)
        assert not fails and len(log) == 1, fails
        want = sn.spectrum(sn.factor_spectra(terms), rig.nz)
        a = np.unravel_index(np.argmax(np.abs(want.imag)), want.shape)
        m = np.minimum(np.arange(N), N - np.arange(N)) ** 2
        n2 = (m[:, None, None] + m[None, :, None] + m[None, None, :])[:, :, :rig.nz]
        b = np.unravel_index(np.argmax(np.where(n2 == n2[a], np.abs(want - want[a]), -1.0)), want.shape)
        conj, swap = good.clone(), good.clone()
        conj[a] = torch.conj(good[a])
        swap[a], swap[b] = good[b], good[a]
        for bad in (conj, swap):
            lg._judge(rig, name, [name], rig.compare(bad, [(1, spec)], rig.nz), log, fails)
        assert len(fails) == 2, (name, log)
