"""GPU: fb_redshift_space on cubes tiled from the constructed lines of sight of tests/rsd_cases.py, every line of the cube
compared on the device with the oracle's result for its pattern, no exceptions allowed.

Line of sight x N + y of the cube holds pattern (x N + y) mod P (P odd: every wave slot of every workgroup meets every pattern),
so the oracle processes P lines while the device processes N^2.  Kernels reached: k_rsd (N = 16, 32: the sorting network;
N = 24, 96: generic plans, the network padded to N2 = 32, 128; method 'cubic' at 16, 24, 64) and k_rsd_cells<T, E> for
E = N / 64 = 1 .. 32 (N = 64 .. 2048) in both precisions.  E = 16 and 32 are the sizes at which the kernel needs more than
64 KiB of LDS (f64 from 1024, f32 at 2048), a lane's occupancy mask reaches 32 bits and, at 2048, the noise index
los N + m passes 2^32.

Bounds (the project's own): double-precision plans 1e-12 max|want|; single-precision plans 2e-6 (max|want| + |want|);
'nearest' equals the oracle's choice exactly; 'cubic' 1e-9 / 3e-6 of the line's max|want|.  A tied grid point may take
either of its two values: grid point 0 of 'rest' (two samples on it) and, for 'nearest', the grid points of 'uniform +3.5'
and grid point N/2 of 'clusters', which are the midpoints of their brackets.  Everywhere else the margins that rsd_cases asserts keep every bracket and every
midpoint clear of both key resolutions, which is what allows zero exceptions.

Supplied noise (N = 64, 512, 1024: E = 1, 8, 16): v = 0, noise = v_pattern / 64, sigma_nl = 64 -- the product is the
pattern's velocity bit for bit, so the same oracle lines and bounds apply.  Device noise (f64 plans, 1024 and 2048): v = 0,
sigma_nl = 3 Hz dz, 2^19 cells on the first and last workgroups and on both sides of los N = 2^32 against the oracle with
the host model's normals (fastbox_amd.rng.los_noise_lines); libm and the device's log / sincos differ in the last bits of a
normal, so, as in test_redshift_space_device_noise_follows_host_model, a 1e-5 share of the cells may lie beyond
1e-9 max|want|.

Memory at 2048 (bound: three quarters of 288 GB): three cubes (density, velocity, result) of 34.4 GB (f32) / 68.7 GB (f64) and
the comparison's temporaries of 2^27 doubles each; asserted from the sizes before anything is allocated."""
import numpy as np
import pytest

from oracle import box_oracle as bo
from tests import rsd_cases as rc
from tests.test_large_grid_reference_gpu import DEVICE_BYTES_BOUND, _Rig

pytestmark = pytest.mark.gpu

METHODS = {"linear": 0, "nearest": 1, "cubic": 2}
CHUNK = 1 << 27                      # elements of one comparison temporary (1 GB in double; at most 3 GB)
TEMPORARIES = 6
NOISE_SIGMA = 64.0
NOISE_SIZES = (64, 512, 1024)
DEVICE_NOISE_SIZES = (1024, 2048)
DEVICE_NOISE_CELLS = 1 << 19
SEED = 0x5DEECE66D2026


def bounds(c, method, precision):
    """(want, bound) tables (P, N) in double of one method: what the device must return and by how much it may miss."""
    w = c["want"][method]
    if method == "nearest":
        return (w.astype(np.float32).astype(np.float64) if precision == "f32" else w), np.zeros_like(w)
    if method == "cubic":
        return w, (1e-9 if precision == "f64" else 3e-6) * np.max(np.abs(w), axis=-1, keepdims=True) * np.ones_like(w)
    if precision == "f64":
        return w, np.full_like(w, 1e-12 * np.max(np.abs(w)))
    return w, 2e-6 * (np.max(np.abs(w)) + np.abs(w))


class Cube(object):
    """The three cubes of one plan and the per-pattern tables they are filled from and compared with."""

    def __init__(self, rig, c):
        self.rig, self.c, self.P, self.N = rig, c, len(c["names"]), rig.N
        N = self.N
        self.per = max(1, CHUNK // N)                                  # lines of sight per chunk
        assert self.per * N * 8 <= 3e9
        self.d, self.v, self.out = rig.new_real(), rig.new_real(), rig.new_real()
        self.fill(self.d, c["d"])
        self.fill(self.v, c["v"])

    def table(self, a, dtype=None):
        t = self.rig.torch
        return t.from_numpy(np.array(a, dtype=np.float64)).to(self.rig.dev).to(dtype or t.float64)

    def pattern(self, l0, l1):
        t = self.rig.torch
        return t.arange(l0, l1, device=self.rig.dev, dtype=t.int64) % self.P

    def spans(self):
        n = self.N * self.N
        return [(l0, min(l0 + self.per, n)) for l0 in range(0, n, self.per)]

    def fill(self, cube, rows):
        """cube[x, y, :] = rows[(x N + y) mod P], exactly (the rows are representable in the plan's type)"""
        tab = self.table(rows, self.rig.rdtype)
        assert np.array_equal(tab.cpu().numpy().astype(np.float64), rows)
        flat = cube.view(self.N * self.N, self.N)
        for l0, l1 in self.spans():
            flat[l0:l1].copy_(tab.index_select(0, self.pattern(l0, l1)))

    def run(self, method, sigma=0.0, noise=None, seed=0):
        self.out.fill_(float("nan"))
        self.rig.call("fb_redshift_space", self.d.data_ptr(), self.v.data_ptr(), noise.data_ptr() if noise is not None else None,
                      self.out.data_ptr(), rc.HZ, float(sigma), seed, METHODS[method], self.rig.stream())

    def worst(self, method):
        """Every line of the result against its pattern's oracle line: per pattern, (largest deviation, largest deviation
        minus bound, number of values that are not finite)."""
        t = self.rig.torch
        want, bound = (self.table(a) for a in bounds(self.c, method, self.rig.precision))
        alt = self.table(self.c["alt_" + method])                      # the other value of a tied grid point
        dev = t.full((self.P,), -np.inf, dtype=t.float64, device=self.rig.dev)
        exc, nonfinite = dev.clone(), t.zeros((self.P,), dtype=t.int64, device=self.rig.dev)
        flat = self.out.view(self.N * self.N, self.N)
        for l0, l1 in self.spans():
            p = self.pattern(l0, l1)
            got = flat[l0:l1].to(t.float64)
            nonfinite.index_add_(0, p, (~t.isfinite(got)).sum(dim=1))
            got.nan_to_num_(nan=1e300, posinf=1e300, neginf=-1e300)
            e = (got - want.index_select(0, p)).abs_()
            e = t.minimum(e, got.sub_(alt.index_select(0, p)).abs_())
            del got
            dev.scatter_reduce_(0, p, e.amax(dim=1), "amax")
            e -= bound.index_select(0, p)
            exc.scatter_reduce_(0, p, e.amax(dim=1), "amax")
            del e
        return dev.cpu().numpy(), exc.cpu().numpy(), nonfinite.cpu().numpy()

    def judge(self, label, method, log, fails):
        dev, exc, nonfinite = self.worst(method)
        bound = bounds(self.c, method, self.rig.precision)[1]
        for name, dv, ex, nf, b in zip(self.c["names"], dev, exc, nonfinite, bound):
            line = "%d %s %-22s %-22s max |got - want| %.3e (bound %.3e .. %.3e)" % (
                self.N, self.rig.precision, label, name, dv, b.min(), b.max())
            log.append(line)
            if nf or not ex <= 0.0:
                fails.append(line + "  beyond its bound by %.3e, %d values not finite" % (ex, nf))


class _Replay(object):
    """Stands in for np.random in the oracle: hands out prepared normals line by line."""

    def __init__(self, rows):
        self.rows = iter(rows)

    def normal(self, mu, sigma, n):
        return next(self.rows)


def noise_lines(N):
    """Lines of sight of the device-noise check: the first and the last workgroups, and the lines either side of the first
    whose noise index los N reaches 2^32 (N = 2048; the middle of the cube otherwise)."""
    n = DEVICE_NOISE_CELLS // N // 4
    half = N * N // 2
    return np.concatenate([np.arange(n), np.arange(half - n, half + n), np.arange(N * N - n, N * N)]).astype(np.int64)


def device_noise(cube, log, fails):
    from fastbox_amd import rng as hostrng
    rig, N, t = cube.rig, cube.N, cube.rig.torch
    z = rc.grid(N)
    sigma = 3.0 * rc.HZ * (z[1] - z[0])
    los = noise_lines(N)
    assert los.size * N >= DEVICE_NOISE_CELLS and np.unique(los).size == los.size
    if N == 2048:
        assert np.sum(los * N >= 2 ** 32) >= los.size // 2 and np.sum(los * N < 2 ** 32) >= los.size // 4
    cube.v.zero_()
    cube.run("linear", sigma=sigma, seed=SEED)
    got = cube.out.view(N * N, N).index_select(0, t.from_numpy(los).to(rig.dev)).cpu().numpy().astype(np.float64)
    d = np.repeat(rc.density(N)[None, :], los.size, axis=0)
    want = bo.redshift_space_density(bo.box_geometry(rc.L, N), d[None], np.zeros_like(d)[None], rc.HZ, sigma,
                                     _Replay(hostrng.los_noise_lines(N, SEED, los)))[0]
    bad = ~(np.abs(got - want) <= 1e-9 * np.max(np.abs(want)))
    line = "%d %s device noise: %d of %d cells beyond 1e-9 max|want| (share %.2e, allowed 1e-5), max |got - want| %.3e" % (
        N, rig.precision, bad.sum(), bad.size, bad.mean(), np.nanmax(np.abs(got - want)))
    log.append(line)
    if not bad.mean() <= 1e-5:
        fails.append(line)
    cube.fill(cube.v, cube.c["v"])


def run_size(N, precision, cubic=False):
    c = rc.lines(N, precision, cubic)
    noise = (not cubic) and N in NOISE_SIZES
    item = 4 if precision == "f32" else 8
    assert (3 + noise) * N ** 3 * item + TEMPORARIES * CHUNK * 8 < DEVICE_BYTES_BOUND
    rig = _Rig(N, precision, L=(rc.L,) * 3)
    log, fails = [], []
    try:
        cube = Cube(rig, c)
        for method in (("cubic",) if cubic else ("linear", "nearest")):
            cube.run(method)
            cube.judge(method, method, log, fails)
        if noise:
            nz = rig.new_real()
            cube.fill(nz, c["v"] / NOISE_SIGMA)
            cube.v.zero_()
            for method in ("linear", "nearest"):
                cube.run(method, sigma=NOISE_SIGMA, noise=nz)
                cube.judge(method + ", supplied noise", method, log, fails)
            del nz
            cube.fill(cube.v, c["v"])
        if not cubic and precision == "f64" and N in DEVICE_NOISE_SIZES:
            device_noise(cube, log, fails)
        del cube
    finally:
        rig.close()
    print("\n".join(log), flush=True)
    assert not fails, "%d of %d comparisons out of bounds:\n%s" % (len(fails), len(log), "\n".join(fails))


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("N", [16, 24, 32, 64, 96, 128, 256, 512, 1024])
def test_constructed_lines(N, precision):
    """linear and nearest, every line of the cube; supplied noise at 64, 512 and 1024; device noise at 1024 (f64)."""
    run_size(N, precision)


def test_constructed_lines_at_2048_single_precision():
    """k_rsd_cells<float, 32>: 80 KiB of LDS per workgroup, 32 cells per lane."""
    run_size(2048, "f32")


def test_constructed_lines_at_2048_double_precision():
    """k_rsd_cells<double, 32>: 144 KiB of LDS per workgroup; linear, nearest and the device noise past index 2^32 on one
    set of buffers (3 x 68.7 GB)."""
    run_size(2048, "f64")


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("N", [16, 24, 64])
def test_constructed_lines_cubic(N, precision):
    """method 'cubic' (k_rsd: sort, tridiagonal solve, evaluation) on the uniform and permute patterns."""
    run_size(N, precision, cubic=True)
