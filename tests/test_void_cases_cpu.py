"""CPU: the constructed cases of tests/void_cases.py against the numpy statement (tests/voids_numpy.py) and, at N = 8-12, the
brute-force walk of tests/test_voids_cpu.py; the property that keeps each case from being vacuous; and the sensitivity of the
comparisons that tests/test_voids_constructed_gpu.py makes: each intended mutation of the statement fails its case."""
import types

import numpy as np
import pytest

from tests import void_cases as vc
from tests import voids_numpy as vn
from tests.test_voids_cpu import _box, brute


def _fields(N):
    f, ins, length = vc.corridor(N)
    return [("corridor", f, ins), ("corridor nan", np.where(ins, f, np.nan), None), ("checkerboard", vc.checkerboard(N), None),
            ("constant", vc.constant(N, -1.25), None), ("signed zeros", vc.signed_zeros(N), None), ("ramp", vc.ramp(N), None)]


@pytest.mark.parametrize("N", [8, 10, 12])
def test_builders_are_the_per_voxel_walk(N):
    for name, f, mask in _fields(N):
        ins = vn.inside(f, mask=mask)
        lab, n = vn.watershed(f, ins)
        blab, bn = brute(f, ins)
        assert n == bn, name
        np.testing.assert_array_equal(lab, blab, err_msg=name)


@pytest.mark.parametrize("N,length,rounds", [(18, 1538, 10), (32, 8447, 13)])
def test_corridor_is_one_long_path(N, length, rounds):
    f, ins, n = vc.corridor(N)
    assert n == length == int(ins.sum())
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f)
    par = vn.descend(f, ins)
    idx = np.arange(N ** 3)
    step = (par >= 0) & (par != idx)
    assert step.sum() == length - 1                                  # one minimum
    assert np.all(f.reshape(-1)[par[step]] == f.reshape(-1)[step] - 1)      # every step is to the next voxel of the corridor
    assert vc.jump_rounds(par) >= rounds
    lab, nreg = vn.watershed(f, ins)
    assert nreg == 1 and int((lab == 1).sum()) == length and np.array_equal(lab > 0, ins)
    # NaN outside instead of a mask: the same labels
    g = np.where(ins, f, np.nan)
    lab2, n2 = vn.watershed(g, vn.inside(g))
    assert n2 == 1 and np.array_equal(lab2, lab)
    # the mask matters: without it the low values outside take every voxel
    lab3, _ = vn.watershed(f, vn.inside(f))
    assert not np.array_equal(lab3, lab)


def test_plateau_and_checkerboard_regions():
    N = 32
    lab, n = vn.watershed(vc.checkerboard(N), np.ones((N, N, N), dtype=bool))
    assert n == N ** 3 // 2 and np.array_equal(np.unique(lab), np.arange(1, n + 1))
    for f in (vc.constant(N, 3.), vc.constant(N, 0.), vc.signed_zeros(N), vc.ramp(N)):
        ins = vn.inside(f)
        lab, n = vn.watershed(f, ins)
        assert n == 1 and np.all(lab == 1)
        assert vn.descend(f, ins)[0] == 0                             # rooted at voxel 0
        assert vn.region_stats(lab, n, f)["argmin"][1] == 0          # the least index of the plateau (-0 is +0)
    assert vc.jump_rounds(vn.descend(vc.constant(N, 3.), np.ones((N, N, N), dtype=bool))) == 7
    z = vc.signed_zeros(N)
    assert np.signbit(z).sum() == N ** 3 // 2 and not z.any()


def test_stripes_end_before_on_and_after_a_wave_boundary():
    for N in (18, 32):
        assert vc.run_end_lanes(N, 63) >= {62, 61} and vc.run_end_lanes(N, 65) >= {0, 1}
        assert vc.run_end_lanes(N, 1) == set(range(64))
        assert vc.run_end_lanes(N, 257) >= {0, 1, 2}                 # 257 = 256 + 1: runs across workgroup boundaries
    assert vc.run_end_lanes(32, 64) == {63}
    assert 63 in vc.run_end_lanes(18, 64) and (18 ** 3) % 64 != 0 and (18 ** 3) % 256 != 0 and (30 ** 3) % 256 != 0
    for run in vc.RUNS:
        lab, n = vc.striped_labels(32, run, 7)
        l = lab.reshape(-1)
        assert n == 7 and l.min() == 1 and l.max() == 7
        ends = np.nonzero(np.diff(l))[0]
        assert np.array_equal(ends, np.arange(run - 1, l.size - 1, run))     # the runs are exactly ``run`` voxels long
        lab, n = vc.striped_labels(32, run, 7, zeros=True)
        assert n == 7 and lab.min() == 0 and np.array_equal(np.nonzero(np.diff(lab.reshape(-1)))[0], ends)
        lab, n = vc.striped_labels(32, run, 7, gaps=True)
        assert n == 21 and np.array_equal(np.unique(lab), np.arange(2, 21, 3))
        st = vn.region_stats(lab, n, vc.dyadic_field(32, 1))
        absent = np.setdiff1d(np.arange(22), np.arange(2, 21, 3))
        assert np.all(st["count"][absent] == 0) and np.all(np.isnan(st["mean"][absent])) and np.all(st["argmin"][absent] == -1)


def _fixed_point_sum(values, B):
    """The device's accumulation of ``values`` under the bound B in exact integer arithmetic: x 2^(93 - e) split into
    floor(v 2^-32) and the rest, each word summed modulo 2^64, then (hi + carry) 2^32 + low word as a double, scaled back."""
    import math
    e = math.frexp(B)[1] if B > 0 else 0
    F = 93 - e
    hi = lo = 0
    for x in values:
        if x == 0.0:
            continue
        v = x * 2.0 ** F
        h = math.floor(v * 2.0 ** -32)
        hi = (hi + int(h)) % 2 ** 64
        lo = (lo + int(round(v - h * 2.0 ** 32))) % 2 ** 64
    h = (hi + (lo >> 32)) % 2 ** 64
    h = h - 2 ** 64 if h >= 2 ** 63 else h
    return math.ldexp(float(h) * 2.0 ** 32 + float(lo & 0xFFFFFFFF), -F)


@pytest.mark.parametrize("N", [18, 32])
def test_dyadic_sums_are_exact_everywhere(N):
    """The argument behind assert_array_equal on the device's sums: with f a multiple of 2^-8 below 2^7 and N <= 32, numpy's
    sequential sums, the exact integer sums and the fixed-point words all hold the same number."""
    lab, n = vc.striped_labels(N, 65, 7)
    f = vc.dyadic_field(N, 3, lab, cancel=4)
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f) and np.max(np.abs(f)) <= 128. and (f < 0).any() and (f > 0).any()
    st = vn.region_stats(lab, n, f)
    ex = vc.exact_sums(lab, n, f)
    for k in ex:
        np.testing.assert_array_equal(st[k], ex[k], err_msg=k)
    assert st["sum"][4] == 0. and st["weight_sum"][4] > 0. and st["count"][4] > 100          # the label that cancels
    assert (st["sum"] < 0).any() and (st["sum"] > 0).any()
    # the fixed-point words, label by label, for sum f and for the index-weighted sum along z
    B = float(np.sum(np.abs(f)))
    l = lab.reshape(-1)
    fl = f.reshape(-1)
    iz = np.arange(N ** 3) % N
    for L in (1, 4, 7):
        sel = l == L
        assert _fixed_point_sum(fl[sel], B) == st["sum"][L]
        assert _fixed_point_sum(np.maximum(-fl[sel], 0.) * iz[sel], B * N) == st["weighted_index_sum"][L, 2]
    # mutation: one run of a stripe dropped, here a run whose values are all zero -- only the counts and index sums can tell
    drop = lab.copy()
    s = 65 * 7 * 3
    assert np.all(l[s:s + 65] == 1)
    drop.reshape(-1)[s:s + 65] = 0
    g = f.copy()
    g.reshape(-1)[s:s + 65] = 0.
    st2, st3 = vn.region_stats(lab, n, g), vn.region_stats(drop, n, g)
    assert np.array_equal(st3["sum"], st2["sum"]) and st3["count"][1] == st2["count"][1] - 65
    assert not np.array_equal(st3["index_sum"], st2["index_sum"])
    # and one run of nonzero values dropped: every exact sum of the label moves
    st4 = vn.region_stats(drop, n, f)
    for k in ("sum", "weight_sum", "weighted_index_sum"):
        assert not np.array_equal(st4[k][1], st[k][1]), k


def test_spike_field():
    N = 32
    f, index = vc.spike_field(N, 5)
    assert f.flat[index] == 2.0 ** 40 and np.array_equal(f.astype(np.float32).astype(np.float64), f)
    assert np.sort(np.abs(f).reshape(-1))[-2] <= 1.0
    import math
    assert math.frexp(float(np.abs(f).sum()))[1] == 41               # one fixed-point unit is 2^(41 - 93) = 2^-52


def _flat_pairs(lab):
    """Mutation: the +z neighbour taken as i + 1 in memory, across the ends of rows."""
    A, B = [], []
    N = lab.shape[0]
    fl = lab.reshape(-1)
    for step in (N * N, N, 1):
        a, b = fl[:-step], fl[step:]
        k = (a > 0) & (b > 0) & (a != b)
        A.append(a[k])
        B.append(b[k])
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def _periodic_pairs(lab):
    """Mutation: a periodic box."""
    A, B = [], []
    for ax in range(3):
        a, b = lab.reshape(-1), np.roll(lab, -1, ax).reshape(-1)
        k = (a > 0) & (b > 0) & (a != b)
        A.append(a[k])
        B.append(b[k])
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def _diagonal_pairs(lab):
    """Mutation: 26-connectivity."""
    A, B = [], []
    N = lab.shape[0]
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1
        if not d.any():
            continue
        sa = tuple(slice(max(0, -k), N - max(0, k)) for k in d)
        sb = tuple(slice(max(0, k), N - max(0, -k)) for k in d)
        a, b = lab[sa].reshape(-1), lab[sb].reshape(-1)
        k = (a > 0) & (b > 0) & (a != b)
        A.append(a[k])
        B.append(b[k])
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def _hand_made(N):
    return [("diagonal", vc.diagonal_labels(N)), ("faces x", vc.face_labels(N, 0)), ("faces y", vc.face_labels(N, 1)),
            ("faces z", vc.face_labels(N, 2)), ("sheet", vc.sheet_labels(N))]


def test_adjacency_cases_and_their_mutations(monkeypatch):
    N = 10
    mean = np.array([np.nan, 1., 1.])
    for name, lab in _hand_made(N):
        assert sorted(np.unique(lab).tolist()) == [0, 1, 2], name
        for thr in (0.5, np.inf):
            out, M = vn.merge(lab, 2, mean, thr)
            assert M == 2 and np.array_equal(out, lab), name
    caught = {}
    for mut, pairs in (("flat", _flat_pairs), ("periodic", _periodic_pairs), ("diagonal", _diagonal_pairs)):
        monkeypatch.setattr(vn, "adjacent_pairs", pairs)
        caught[mut] = [name for name, lab in _hand_made(N) if vn.merge(lab, 2, mean, np.inf)[1] != 2]
    monkeypatch.undo()
    assert "faces z" in caught["flat"] and "faces y" in caught["flat"]
    assert caught["periodic"] == ["faces x", "faces y", "faces z", "sheet"]       # the sheet case has label 1 at ix = 0, 2 at N - 1
    assert caught["diagonal"] == ["diagonal"]
    # label 0 blocks: the sheet merges once the 0 is a region like any other
    lab = vc.sheet_labels(N) + 1
    assert vn.merge(lab, 3, np.array([np.nan, 1., 1., 1.]), np.inf)[1] == 1


@pytest.mark.parametrize("order", vc.ORDERS)
def test_chain_is_one_component(order):
    N = 32
    n = N * N
    o = vc.chain_order(n, order)
    assert np.array_equal(np.sort(o), np.arange(1, n + 1))
    if order == "zigzag":
        assert o[:4].tolist() == [1, n, 2, n - 1]
    lab, f, nl = vc.chain_labels(N, order)
    assert nl == n and np.array_equal(np.unique(lab), np.arange(1, n + 1)) and np.all(lab == lab[:, :, :1])
    st = vn.region_stats(lab, n, f)
    a, b = vn.adjacent_pairs(lab)
    d = np.abs(st["mean"][a] - st["mean"][b])
    assert np.all((d == 1.) | (d >= 3.)) and np.unique(np.minimum(a, b)[d == 1.] * (n + 1) + np.maximum(a, b)[d == 1.]).size == n - 1
    out, M = vn.merge(lab, n, st["mean"], 1.5)
    assert M == 1 and np.all(out == 1)
    assert vn.merge(lab, n, st["mean"], 0.)[1] == n
    assert vn.merge(lab, n, st["mean"], np.inf)[1] == 1
    # one interface exactly at the threshold: strict, so two components; <= (the next threshold up) joins them
    k = n // 2 + 5
    lab, f, _ = vc.chain_labels(N, order, equal_at=k)
    st = vn.region_stats(lab, n, f)
    a, b = vn.adjacent_pairs(lab)
    d = np.abs(st["mean"][a] - st["mean"][b])
    assert (d == 1.5).sum() == N and np.all((d == 1.) | (d == 1.5) | (d >= 2.5))
    out, M = vn.merge(lab, n, st["mean"], 1.5)
    assert M == 2
    lo = o[:k].min() < o[k:].min()
    assert np.array_equal(out == 1, np.isin(lab, o[:k] if lo else o[k:]))
    assert vn.merge(lab, n, st["mean"], np.nextafter(1.5, 2.))[1] == 1


def test_merge_counts_absent_labels():
    lab, n = vc.striped_labels(16, 65, 5, zeros=True, gaps=True)
    st = vn.region_stats(lab, n, vc.dyadic_field(16, 2))
    out, M = vn.merge(lab, n, st["mean"], 0.)
    assert M == n == 15 and np.array_equal(out, lab)


def test_linear_stacking_tells_the_axes_apart():
    N = 12
    box = _box(N, (1e3, 7e2, 1.3e3))
    coef = (3., -5., 7., 11.)
    f = vc.linear_field(coef, box)
    lab = np.ones((N, N, N), dtype=np.int32)
    cen = np.array([[400., 0., 0.], [450., -200., 100.], [300., 0., 600.]])          # the grid's +x side leaves the box
    rad = np.array([200., 150., 300.])
    o, fail, cnt = vn.stack(lab, f, [1, 1, 1], cen, rad, box, 1., 7)
    want, wcnt = vc.linear_stack(coef, cen, rad, box, 1., 7)
    np.testing.assert_array_equal(cnt, wcnt)
    assert 0 < (cnt == 0).sum() and (cnt == 3).any() and (cnt == 1).any() and fail == []
    m = cnt > 0
    scale = np.max(np.abs(f))
    assert np.max(np.abs(o.data[m] - want[m])) <= 1e-12 * scale
    # grid[a] and grid[b] swapped: the values move by far more than the bound
    swapped, scnt = vc.linear_stack(coef, cen, rad, box, 1., 7, swap=True)
    both = m & (scnt > 0)
    assert np.max(np.abs(o.data[both] - swapped[both])) > 1e-3 * scale
    # u exactly N - 2 is the last valid cell, N - 1 is outside, and the double just below N - 1 is still inside
    x0, dx = vn.axes(box)
    for axis in range(3):
        for k in (N - 2, N - 1):
            below, at = vc.edge_u(box, axis, k)
            assert (at - x0[axis]) / dx[axis] == k and np.nextafter(below, np.inf) == at
            for coord, valid in ((at, k == N - 2), (below, True)):
                c = np.zeros(3)
                c[axis] = coord
                _, fail, cnt = vn.stack(lab, f, [1], c[None], np.zeros(1), box, 1., 1)
                assert bool(cnt[0, 0, 0]) is valid and (fail == []) is valid


def test_watershed_refuses_a_box_of_2_to_the_31_voxels():
    from fastbox_amd import voids
    eng = types.SimpleNamespace(N=1291)
    with pytest.raises(ValueError, match="2\\^31"):
        voids._watershed(eng, None, voids.MASK_ALL, 0., None)
    assert 1290 ** 3 < 2 ** 31 <= 1291 ** 3 and voids.MAX_WATERSHED_N == 1290
