"""CPU: the LSSA statement (tests/lssa_numpy.py) and the host functions of fastbox_amd.inpaint against vectors recorded from the
reference (tests/golden/lssa_n16.npz, tools/make_golden_lssa.py), and the argument checks, which precede the device.

(a) lssa_pspec on the recorded amplitudes against the recorded ps: within 10 delta_ref (floor 1e-12) of max|ps|, delta_ref the
    deviation of the statement's two evaluations.  No optimiser is involved.
(b) The closed-form amplitudes against the reference's fitted ones, within ten times the largest deviation the generator
    printed per form, relative to max|A| of the row.  Printed (SciPy 1.15.3, L-BFGS-B, four rows):
        real / imaginary form:   1.15e-07, 6.73e-08, 5.79e-08, 3.34e-08   -> bound 1.15e-06
        amplitude / phase form:  2.34e-02, 5.96e-02, 3.91e-02, 5.15e-06   -> bound 5.96e-01
    The amplitude / phase figures of rows 0-2 come from one mode each and are not a stopping error: the reference bounds the
    phase to [0, 2 pi] and starts at pi / 2, so a mode whose optimum lies just below 2 pi ends on the bound at 0 (row 0, mode
    14: phase 6.26), and a mode with a small amplitude (the Nyquist mode of rows 1 and 2) stays at amp = 0, where the phase
    has no gradient.  Every other mode of that form agrees to 6e-5 or better.  The form is compared in the complex plane,
    amp e^{i phase}: the optimiser returns negative amplitudes with the phase shifted by pi.
(c) trim_flagged_channels and lssa_decorr_matrix against recorded values; ps from trimmed and untrimmed flags agree."""
import os
import types

import numpy as np
import pytest

from fastbox_amd import inpaint
from tests import lssa_numpy as ls

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lssa_n16.npz")
FLOOR = 1e-12
BOUND_RI = 10. * 1.15e-07
BOUND_AP = 10. * 5.96e-02


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def _statement(g, r, via="direct"):
    return ls.statement(g["d"][r:r + 1], g["w"][r:r + 1].astype(np.float64), g["var"][r:r + 1], g["taper"][r:r + 1], g["tau"],
                        g["freqs"], via=via)


def test_pspec_of_recorded_amplitudes_matches_the_reference(g):
    for r in range(4):
        w = g["w"][r].astype(np.float64)
        _, _, Scc, Scs, Sss = _sums(w, g["tau"], g["freqs"], "direct")
        a = ls.power(g["A_re"][r], g["A_im"][r], Scc, Scs, Sss)
        b = ls.power(g["A_re"][r], g["A_im"][r], *_sums(w, g["tau"], g["freqs"], "alt")[2:])
        dref, big = ls.delta_ref(a, b)
        bound = max(10. * dref, FLOOR) * big
        for what, got in (("statement", a), ("inpaint.lssa_pspec", inpaint.lssa_pspec(g["A_re"][r], g["A_im"][r], w, g["tau"], g["freqs"]))):
            dev = float(np.max(np.abs(got - g["ps"][r])))
            assert dev <= bound, "row %d, %s: deviation %.3e (relative to max|ps|), delta_ref %.3e" % (r, what, dev / big, dref)


def _sums(w, tau, freqs, via):
    """S_cc, S_cs, S_ss of one spectrum through the statement (with unit data)"""
    phi = ls.phase(tau, freqs)
    if via == "direct":
        c, s = w * np.cos(phi), w * np.sin(phi)
        return None, None, np.sum(c * c, axis=1), np.sum(c * s, axis=1), np.sum(s * s, axis=1)
    w2 = (w * w)[::-1]
    c2, s2 = np.cos(2. * phi)[:, ::-1], np.sin(2. * phi)[:, ::-1]
    return None, None, 0.5 * np.sum(w2 * (1. + c2), axis=1), 0.5 * np.sum(w2 * s2, axis=1), 0.5 * np.sum(w2 * (1. - c2), axis=1)


def test_closed_form_amplitudes_match_the_fitted_ones(g):
    for r in range(4):
        a_re, a_im, _, _ = _statement(g, r)
        A = a_re[0] + 1j * a_im[0]
        big = float(np.max(np.abs(A)))
        dev_ri = float(np.max(np.abs(g["A_re"][r] + 1j * g["A_im"][r] - A))) / big
        dev_ap = float(np.max(np.abs(g["amp"][r] * np.exp(1j * g["phase"][r]) - A))) / big
        print("row %d: real / imaginary %.3e, amplitude / phase %.3e" % (r, dev_ri, dev_ap))
        assert dev_ri <= BOUND_RI, "row %d, real / imaginary form: %.3e" % (r, dev_ri)
        assert dev_ap <= BOUND_AP, "row %d, amplitude / phase form: %.3e" % (r, dev_ap)
        # the two evaluations of the statement agree to rounding
        b_re, b_im, _, _ = _statement(g, r, "alt")
        assert np.max(np.abs(b_re - a_re)) <= 1e-14 * big and np.max(np.abs(b_im - a_im)) <= 1e-14 * big


def test_trim_and_decorr_matrix_match_the_reference(g):
    w2 = g["w"][2].astype(np.float64)
    assert np.array_equal(inpaint.trim_flagged_channels(w2, g["d"][2]), g["trim_1d"])
    assert np.array_equal(inpaint.trim_flagged_channels(w2, g["trim_in"]), g["trim_2d"])
    with pytest.raises(ValueError):
        inpaint.trim_flagged_channels(w2, g["d"][2][:5])
    for r in range(4):
        w = g["w"][r].astype(np.float64)
        for n in range(16):
            rot, eig = inpaint.lssa_decorr_matrix(w, g["tau"][n], g["freqs"])
            assert np.array_equal(rot, g["rot"][r, n]) and np.array_equal(eig, g["eig"][r, n]), (r, n)
        # trimmed flags and frequencies give the same power (the reference's own agree to 6.8e-16 of max|ps| on these rows)
        keep = w == 1.
        a = inpaint.lssa_pspec(g["A_re"][r], g["A_im"][r], w, g["tau"], g["freqs"])
        b = inpaint.lssa_pspec(g["A_re"][r], g["A_im"][r], w[keep], g["tau"], g["freqs"][keep])
        dev = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        assert dev <= 1e-14, "row %d: trimmed against untrimmed %.3e" % (r, dev)
        assert float(np.max(np.abs(g["ps"][r] - g["ps_trim"][r])) / np.max(np.abs(g["ps"][r]))) <= 1e-14
    # without the decorrelation: |A|^2 (the reference ignores the argument)
    assert np.array_equal(inpaint.lssa_pspec(g["A_re"][0], g["A_im"][0], g["w"][0], g["tau"], g["freqs"], decorrelate_amps=False),
                          g["A_re"][0] ** 2. + g["A_im"][0] ** 2.)


def test_default_tau_is_the_reference_expression():
    f = ls.case_freqs(16)
    assert np.array_equal(inpaint.lssa_tau(f), np.fft.fftfreq(n=16, d=f[1] - f[0]) * 1e3)
    assert inpaint.lssa_tau(f)[1] < 0.                                 # descending frequencies: the sign is kept
    assert np.array_equal(inpaint.lssa_phase(inpaint.lssa_tau(f), f)[3], 2. * np.pi * inpaint.lssa_tau(f)[3] * f / 1e3)


def test_a_fully_flagged_row_in_the_statement():
    c = ls.build_case(16, True)
    a_re, a_im, ps, G = ls.statement(np.where(c["w"] != 0., c["d"], 0.)[:8], c["w"][:8], None, None, ls.case_tau(16, 5), c["freqs"])
    assert G[3] == 0. and np.all(a_re[3] == 0.) and np.all(a_im[3] == 0.) and np.all(np.isnan(ps[3]))
    assert not np.isnan(np.delete(ps, 3, axis=0)).any()
    mean, err, n = ls.averages(ps, G)
    assert n == 7 and np.all(np.isfinite(mean)) and np.all(np.isfinite(err))


def test_argument_errors_precede_the_device():
    N = 16
    f = ls.case_freqs(N)
    box = types.SimpleNamespace(engine=types.SimpleNamespace(N=N), freq_array=lambda: f)
    d, w = np.zeros((N * N, N)), np.ones((N * N, N))
    for fn in (inpaint.lssa_fit_modes, inpaint.lssa_delay_spectrum):
        with pytest.raises(ValueError):
            fn(d[:, :8], w, box=box)
        with pytest.raises(ValueError):
            fn(d, w[:100], box=box)
        with pytest.raises(ValueError):
            fn(d, np.ones(N - 1), box=box)
        with pytest.raises(ValueError):
            fn(d, w, tau=np.zeros(0), box=box)
        with pytest.raises(ValueError):
            fn(d, w, tau=np.zeros(1025), box=box)
        with pytest.raises(ValueError):
            fn(d, w, tau=np.zeros((2, 2)), box=box)
        bad = f.copy()
        bad[3] = bad[2]
        with pytest.raises(ValueError):
            fn(d, w, freqs=bad, box=box)
        with pytest.raises(ValueError):
            fn(d, w, freqs=f[:8], box=box)
        with pytest.raises(ValueError):
            fn(d, w, taper=np.ones(N + 1), box=box)
        with pytest.raises(ValueError):
            fn(d, w, N=np.ones(N + 1), box=box)
        with pytest.raises(NotImplementedError):
            fn(d + 1j, w, box=box)
        with pytest.raises(TypeError):
            fn(d, w)
    with pytest.raises(TypeError):
        inpaint.lssa_pspec(np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError):
        inpaint.lssa_pspec(np.zeros(4), np.zeros(3), np.ones(N), np.zeros(4), f)
