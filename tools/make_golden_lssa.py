"""Golden vectors of the LSSA half of the reference's fastbox/inpaint.py (trim_flagged_channels, lssa_fit_modes in both forms,
lssa_decorr_matrix, lssa_pspec) for tests/test_lssa_cpu.py.  Loads the reference module by path (it needs only numpy and
SciPy), so it runs only where the reference sources are present; the output is committed under tests/golden/.

    python tools/make_golden_lssa.py <path of the reference's fastbox/inpaint.py>

lssa_n16.npz holds one 16-channel case of four rows over descending frequencies: row 0 unflagged, row 1 with a run of four
flags, row 2 with random flags, row 3 with random flags, a Hann taper and unequal variances.  Per row the reference is handed the
trimmed spectrum, diag(1 / var) of the unflagged channels, an explicit taper (its default False raises AttributeError) and
tau / 1e3 (its fit lacks the / 1e3 of its lssa_decorr_matrix).  Recorded: d, w, var, taper, freqs, tau; A_re, A_im (real /
imaginary form) and amp, phase (amplitude / phase form) of lssa_fit_modes; ps = lssa_pspec(A_re, A_im, w, tau, freqs) with
the untrimmed w and freqs and ps_trim with the trimmed ones; rot, eig = lssa_decorr_matrix(w, tau_n, freqs) of every row and
mode; trim_1d = trim_flagged_channels(w, d) of row 2 and trim_2d of a 16 x 16 matrix (trim_in) under row 2's flags; dev_ri,
dev_ap: the deviation of the fitted amplitudes from the closed form (tests/lssa_numpy.py) relative to max|A| of the row, the
optimiser's own stopping error.  It prints those deviations: the bounds of the test are ten times the largest per form."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lssa_numpy as ls                                             # noqa: E402


def load_inpaint(path):
    spec = importlib.util.spec_from_file_location("reference_inpaint", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(mod, N=16):
    rs = np.random.RandomState(20240611)
    freqs = ls.case_freqs(N)
    tau = np.fft.fftfreq(n=N, d=freqs[1] - freqs[0]) * 1e3
    d = rs.standard_normal((4, N)) + 0.7 * np.cos(ls.phase(tau[2:3], freqs)[0] + 0.3)
    w = np.ones((4, N))
    w[1, 6:10] = 0.
    w[2, rs.choice(N, size=4, replace=False)] = 0.
    w[3, rs.choice(N, size=3, replace=False)] = 0.
    var = np.ones((4, N))
    var[3] = rs.uniform(0.5, 2.0, size=N)
    taper = np.ones((4, N))
    taper[3] = np.hanning(N)
    out = dict(d=d, w=w.astype(np.int8), var=var, taper=taper, freqs=freqs, tau=tau)
    names = ("A_re", "A_im", "amp", "phase", "ps", "ps_trim")
    rec = {k: np.zeros((4, N)) for k in names}
    rot, eig = np.zeros((4, N, 2, 2)), np.zeros((4, N, 2))
    dev_ri, dev_ap = np.zeros(4), np.zeros(4)
    for r in range(4):
        wr = w[r]
        dt, ft = mod.trim_flagged_channels(wr, d[r]), mod.trim_flagged_channels(wr, freqs)
        tt, vt = mod.trim_flagged_channels(wr, taper[r]), mod.trim_flagged_channels(wr, var[r])
        invcov = np.diag(1. / vt)
        _, rec["A_re"][r], rec["A_im"][r] = mod.lssa_fit_modes(dt, ft, invcov=invcov, fit_amp_phase=False, tau=tau / 1e3, taper=tt)
        _, rec["amp"][r], rec["phase"][r] = mod.lssa_fit_modes(dt, ft, invcov=invcov, fit_amp_phase=True, tau=tau / 1e3, taper=tt)
        rec["ps"][r] = mod.lssa_pspec(rec["A_re"][r], rec["A_im"][r], wr, tau, freqs)
        rec["ps_trim"][r] = mod.lssa_pspec(rec["A_re"][r], rec["A_im"][r], mod.trim_flagged_channels(wr, wr), tau, ft)
        for n in range(N):
            rot[r, n], eig[r, n] = mod.lssa_decorr_matrix(wr, tau[n], freqs)
        a_re, a_im, _, _ = ls.statement(d[r:r + 1], wr[None], var[r:r + 1], taper[r:r + 1], tau, freqs)
        A = a_re[0] + 1j * a_im[0]
        big = np.max(np.abs(A))
        dev_ri[r] = np.max(np.abs(rec["A_re"][r] + 1j * rec["A_im"][r] - A)) / big
        dev_ap[r] = np.max(np.abs(rec["amp"][r] * np.exp(1j * rec["phase"][r]) - A)) / big
        print("row %d: the reference's fit deviates from the closed form by %.2e (real / imaginary form), %.2e (amplitude / "
              "phase form), relative to max|A|; ps trimmed against untrimmed: %.2e" % (
                  r, dev_ri[r], dev_ap[r], np.max(np.abs(rec["ps"][r] - rec["ps_trim"][r])) / np.max(np.abs(rec["ps"][r]))))
    print("largest: %.2e (real / imaginary), %.2e (amplitude / phase)" % (dev_ri.max(), dev_ap.max()))
    trim_in = rs.standard_normal((N, N))
    out.update(rec)
    out.update(rot=rot, eig=eig, dev_ri=dev_ri, dev_ap=dev_ap, trim_in=trim_in,
               trim_1d=mod.trim_flagged_channels(w[2], d[2]), trim_2d=mod.trim_flagged_channels(w[2], trim_in))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = load_inpaint(sys.argv[1])
    out = os.path.join(ROOT, "tests", "golden", "lssa_n16.npz")
    np.savez_compressed(out, **make(mod))
    print("wrote", out)


if __name__ == "__main__":
    main()
