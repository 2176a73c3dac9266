"""CPU: the constructed lines of sight of tests/rsd_cases.py are what they claim to be -- the margins that make their brackets
unambiguous hold for every size and both precisions, each pattern holds the feature it was built for (one key per cell, a
whole line in one cell, two clusters 57 lanes apart, exact hits beside second keys, a permutation), and the closed forms agree
with the oracle.  Also fastbox_amd.rng.los_noise_lines against los_noise."""
import numpy as np
import pytest

from fastbox_amd import rng as hostrng
from tests import rsd_cases as rc

PRECISIONS = ("f64", "f32")


def _cells(N, v):
    return np.floor(rc.positions(N, v) + 1e-9).astype(int)          # (an exact hit may sit a rounding below its grid point)


@pytest.mark.parametrize("N", rc.SIZES)
def test_density_line(N):
    d = rc.density(N)
    assert np.array_equal(d, d.astype(np.float32)) and np.array_equal(8 * d, np.rint(8 * d)) and np.abs(d).max() <= 32
    assert np.all(d[1:] != d[:-1]) and d[0] != d[-1]
    assert 0.5 * (d[0] + d[-1]) == rc.FILL and not np.any(d == rc.FILL)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", rc.SIZES)
def test_margins_of_every_pattern(N, precision):
    """(i) distinct keys and grid points 2^-12 cell apart, (ii) brackets of a grid point 1/8 cell apart, (iii) their midpoint
    2^-12 cell from the grid point, but for uniform +3.5, whose every grid point is one, and grid point N/2 of clusters; the exact hits are those of rest
    (all) and alternate (the even samples) only."""
    for cubic in (False, True):
        c = rc.lines(N, precision, cubic)
        assert len(c["names"]) % 2 == 1 and len(set(c["names"])) == len(c["names"])
        for name, v in zip(c["names"], c["v"]):
            gap, off_grid, bracket, mid, hits = rc.margins(N, name, v)
            ties = rc.midpoint_ties(N, v)
            print("N = %4d %s %-22s key gap %.3e  key to grid point %.3e  bracket %.3e  midpoint to grid point %.3e  exact hits %d  "
                  "midpoint ties %d" % (N, precision, name, gap, off_grid, bracket, mid, hits, len(ties)))
            assert gap >= rc.MARGIN and off_grid >= rc.MARGIN and bracket >= rc.BRACKET, name
            if name == "uniform +3.5":
                assert mid < 1e-6 and sorted(ties) == [1, 2, 3] + list(range(5, N - 1))   # keys at 0.5 .. N - 1.5 and 3.875
            elif name == "clusters":                                  # facing ends at 3E + (N-1)/(N+1) and N - 3E - 1 + 2/(N+1)
                assert mid < 1e-4 and sorted(ties) == [N // 2]
            else:
                assert mid >= rc.MARGIN and not ties, name
            assert hits == {"rest": N, "alternate": N // 2}.get(name, 0), name


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", rc.SIZES)
def test_patterns_hold_their_feature(N, precision):
    c = rc.lines(N, precision)
    row = dict(zip(c["names"], c["v"]))
    E = rc.cells_per_lane(N)
    assert np.array_equal(row["rest"], np.zeros(N))
    p = rc.positions(N, row["rest"])
    assert p[0] == 0. and p[N - 1] == 0. and np.array_equal(np.rint(p[1:N - 1]), np.arange(1, N - 1))    # the one tie
    for a in rc.UNIFORM:                                             # one key per cell, sample N-1 3/8 cell past sample 0
        cell = _cells(N, row["uniform " + a])
        p = rc.positions(N, row["uniform " + a])
        assert np.unique(cell[:N - 1]).size == N - 1
        assert abs((p[N - 1] - p[0]) % (N - 1) - 0.375) < 1e-3
    assert np.any(np.diff(_cells(N, row["uniform -(N/2+1/4)"])[:N - 1]) < 0)                   # wraps inside the line
    cc = rc.collapse_cells(N)
    assert len(set(cc)) == 4 and cc[0] == 0 and cc[-1] == N - 2 and (N % 64 or cc[2] == 31 * E + E - 1)
    assert N < 128 or N % 64 or cc[1] % E == E - 1                   # a lane's last cell
    for c0 in cc:
        assert np.all(_cells(N, row["collapse %d" % c0]) == c0)
    lo, hi = rc.cluster_cells(N)
    cell = _cells(N, row["clusters"])
    assert np.all(cell[0::2] == lo) and np.all(cell[1::2] == hi) and 0 < lo < hi < N - 2
    assert N % 64 or (lo == 3 * E and hi == 60 * E + E - 1 and hi // E - lo // E == 57)
    cell = _cells(N, row["alternate"])
    p = rc.positions(N, row["alternate"])
    assert np.all(np.bincount(cell, minlength=N)[2:N - 1:2] == 2) and np.all(np.bincount(cell, minlength=N)[3:N:2] == 0)
    assert np.bincount(cell)[0] == 1 and np.bincount(cell)[1] == 1 and abs(p[N - 1] - 1.5) < 1e-6
    for s in (1, 2):
        cell = _cells(N, row["permute %d" % s])
        assert np.array_equal(np.sort(cell[:N - 1]), np.arange(N - 1)) and cell[N - 1] == cell[0]
        assert N < 64 or np.mean(np.abs(np.diff(cell[:N - 1])) > E) > 0.5               # no ordered run


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", rc.SIZES)
def test_closed_forms_against_the_oracle(N, precision):
    """collapse: fill everywhere, nearest d[0] up to c0 and d[N-1] above; rest: the samples, fill at the last grid point;
    uniform +1/4: fill at both ends, 3/4 d[m-1] + 1/4 d[m] between.  Fill counts of the others are recorded."""
    c = rc.lines(N, precision)
    d = rc.density(N)
    lin, near = c["want"]["linear"], c["want"]["nearest"]
    assert lin.shape == (len(c["names"]), N) and np.all(np.isfinite(lin)) and np.all(np.isfinite(near))
    fills = {}
    for r, name in enumerate(c["names"]):
        p = rc.positions(N, c["v"][r])
        outside = (np.arange(N) < p.min() - 1e-9) | (np.arange(N) > p.max() + 1e-9)     # np.interp's out-of-range rule
        nfill = fills[name] = int(outside.sum())
        assert np.all(lin[r, outside] == rc.FILL), name
        assert np.all(np.isin(near[r], d)), name                     # nearest copies samples
        if name.startswith("collapse"):
            c0 = int(name.split()[1])
            assert nfill == N, name
            assert np.all(near[r, :c0 + 1] == d[0]) and np.all(near[r, c0 + 1:] == d[N - 1]), name
        if name == "rest":
            assert np.array_equal(lin[r, 1:N - 1], d[1:N - 1]) and lin[r, N - 1] == rc.FILL and lin[r, 0] in (d[0], d[N - 1])
            assert np.array_equal(near[r, 1:N - 1], d[1:N - 1]) and near[r, N - 1] == d[N - 2]
            for m in ("linear", "nearest"):
                assert {c["want"][m][r, 0], c["alt_" + m][r, 0]} == {d[0], d[N - 1]}
                assert np.array_equal(c["alt_" + m][r, 1:], c["want"][m][r, 1:])
        else:
            assert np.array_equal(c["alt_linear"][r], lin[r])
            differs = np.flatnonzero(c["alt_nearest"][r] != near[r])
            if name == "uniform +3.5":                               # either neighbour, and they differ
                assert sorted(differs) == [1, 2, 3] + list(range(5, N - 1)) and np.all(np.isin(c["alt_nearest"][r], d))
            elif name == "clusters":
                assert list(differs) == [N // 2] and {near[r, N // 2], c["alt_nearest"][r, N // 2]} == {d[N - 2], d[1]}
            else:
                assert differs.size == 0, name
        if name == "uniform +1/4":
            assert lin[r, 0] == rc.FILL and lin[r, N - 1] == rc.FILL and nfill == 2
            mid = 0.25 * d[1:N - 2] + 0.75 * d[2:N - 1]               # grid point m between samples m-1 (at m - 3/4) and m (at m + 1/4)
            assert np.max(np.abs(lin[r, 2:N - 1] - mid)) < (1e-9 if precision == "f64" else 1e-4)
        if name == "clusters":
            lo, hi = rc.cluster_cells(N)
            assert nfill == N - (hi - lo) and np.all(lin[r, :lo + 1] == rc.FILL) and np.all(lin[r, hi + 1:] == rc.FILL)
            assert set(near[r]) == {d[0], d[N - 2], d[1], d[N - 1]}   # below, the clusters' facing ends, above
        if name == "alternate":
            assert nfill == 1 and lin[r, N - 1] == rc.FILL
            assert np.max(np.abs(lin[r, 0:N - 1:2] - d[0:N - 1:2])) < 1e-9                       # the exact hits
        if name.startswith("permute"):
            assert nfill == 2 and outside[0] and outside[N - 1]                                  # no key at fraction 0
    print("N = %4d %s fill counts: %s" % (N, precision, fills))


def test_cubic_lines_against_the_oracle():
    for N in (16, 24, 64):
        for precision in PRECISIONS:
            c = rc.lines(N, precision, cubic=True)
            assert set(c["want"]) == {"cubic"} and np.all(np.isfinite(c["want"]["cubic"]))
            assert not any(n.split()[0] in ("rest", "collapse", "clusters", "alternate") for n in c["names"])


@pytest.mark.parametrize("N", [6, 16, 2048])
def test_los_noise_lines(N):
    seed = 0x1234567890ABCDEF
    if N <= 16:
        full = hostrng.los_noise(N, seed).reshape(N * N, N)
        pick = [0, 1, N, N * N - 1, 7]
        assert np.array_equal(hostrng.los_noise_lines(N, seed, pick), full[pick])
        assert np.array_equal(hostrng.los_noise_lines(N, seed, pick, np.float32), hostrng.los_noise(N, seed, np.float32).reshape(N * N, N)[pick])
        return
    # beyond 2^32 elements: the same calls as the stream's definition (call = element >> 2, output = element & 3)
    los = N * N - 1
    assert los * N >= 2 ** 32
    got = hostrng.los_noise_lines(N, seed, [los])
    o = hostrng._call(np.arange(los * N // 4, (los + 1) * N // 4, dtype=np.uint64), 1, seed, 0)
    want = np.stack(hostrng.box_muller(o[0], o[1]) + hostrng.box_muller(o[2], o[3]), axis=-1).reshape(1, N)
    assert np.array_equal(got, want) and abs(got.std() - 1.) < 0.1
