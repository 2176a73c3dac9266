"""GPU: the 512^3, 1024^3 and 2048^3 kernels against references that do not come from this library.

Transforms (through the C ABI, on torch tensors' device pointers and torch's current stream, as fastbox_amd.distributed.HipSlabOps
does): every case of tests/separable_numpy.py is built on the device from its factor vectors, exactly (8-bit factors), and
EVERY output element is compared, in fp64 over chunks of x-planes, with the outer product of the factors' 1-D transforms (formed
on the host in long double and rounded once to double).  fb_fft_r2c, fb_fft_c2r (called directly: it destroys its input; and
through Engine.fft_c2r(destroy=False), after which the input must be bit for bit what it was) and fb_fft_c2c in both directions.
The input of the inverse transforms is the reference spectrum rounded to the plan's storage type; by Parseval that rounding moves
the field by at most eps rms(field) in the rms, which is added to the rms bound of those entry points.  Bounds: separable_numpy's
docstring; the reference's own error (three correctly rounded factors, two complex products, the sum of the terms: < 8 units
of 2^-53 of the result) is added to every bound.

Memory (MI355X: 288 GB; three quarters = 216 GB), from the sizes, N = 2048:
  f32: real 2048^3 x 4 = 34.4 GB, half 2048 x 2049 x 1040 x 8 = 34.9 GB, the non-destroying c2r's copy and result are not taken
       at this size (fb_fft_c2r is called directly); c2c: the full complex buffer 2048^3 x 8 = 68.7 GB beside a comparison chunk
       of < 3 GB (real and half buffers released first): run.
  f64: real 68.7 GB + half 69.8 GB + chunk < 3 GB = 142 GB: r2c and the destroying c2r run.  c2c (137 GB for the buffer alone) is
       not asked for at this size.
At 2048^3 in single precision r2c and c2r also run with the other row form (fb_set_tile_rows(64)) and the other schedule
(fb_set_pass_schedule(0, 0, 0)) of the strided passes.

Generator (rng='device', fixed seed, realisations 0 and 1) at 1024^3 (f32, f64, and in f32 a cuboid box, which takes the
fb_set_amplitude_sym table) and 2048^3 (f32), on whole k_z planes -- all k_x, k_y; k_z in {0, 1, N/2 - 1, N/2} and four seeded
ones -- against the host model fastbox_amd.rng.half_spectrum_noise x sqrt(P boxfactor):
  (a) fb_colour_device's half spectrum, per mode, to tol amp (1 + |z|), tol = 3e-5 (f32) / 1e-11 (f64) (test_box_gpu.py);
  (b) the fused route of realise_density() (fb_realise_density_begin + _finish: k_fft_strided<N, GEN>, the y and z passes)
      followed by fb_fft_r2c, which the transform tests have verified on its own: per mode to tol rms(|z amp| over the plane)
      sqrt(log2 N^3 / log2 512^3): the rounding of the two transforms is white across modes;
  (c) the planes contain the corners of the cube -- |k| up to the last entry of the cubic box's shell table, n^2 = 3 (N/2)^2 --
      and, at 2048, modes whose Philox call index ((k_x mod N/2) N + k_y)(N/2 + 1) + k_z is >= 2^31: both asserted."""
import ctypes
import gc

import numpy as np
import pytest

from oracle import standin
from tests import separable_numpy as sn

pytestmark = pytest.mark.gpu

REF_ERR = 8.0 * 2.0 ** -53
GEN_TOL = {"f32": 3e-5, "f64": 1e-11}
DEVICE_BYTES_BOUND = 0.75 * 288e9
SEED = 20261


class _Rig(object):
    """An Engine and the torch tensors its entry points are called on."""

    def __init__(self, N, precision, L=(1e3, 1e3, 1e3), engine=None):
        import torch
        from fastbox_amd import _lib, hostgeom
        from fastbox_amd.device import Engine
        self.torch, self.lib = torch, _lib
        self.N, self.H, self.nz, self.precision = N, N // 2, N // 2 + 1, precision
        self.dev = torch.device("cuda", 0)
        if engine is None:
            axis2, ksc, kpar = hostgeom.axis_tables(N, L)
            engine = Engine(N, L, axis2, ksc, kpar, np.linspace(-0.5 * L[2], 0.5 * L[2], N), precision=precision)
        self.eng = engine
        self.rdtype = torch.float32 if precision == "f32" else torch.float64

    def close(self):
        self.torch.cuda.synchronize()
        self.eng.close()
        gc.collect()
        self.torch.cuda.empty_cache()

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def call(self, name, *args):
        self.lib.call(name, self.eng._plan, *args)

    def new_real(self):
        return self.torch.empty((self.N,) * 3, dtype=self.rdtype, device=self.dev)

    def new_half(self):
        return self.torch.zeros((self.N, self.eng.rows, self.eng.pitch, 2), dtype=self.rdtype, device=self.dev)

    def new_full(self):
        return self.torch.empty((self.N,) * 3 + (2,), dtype=self.rdtype, device=self.dev)

    def half_view(self, half):
        return self.torch.view_as_complex(half)[:, :self.N, :self.nz]

    def chunks(self, nlast):
        per = max(1, (1 << 25) // (self.N * nlast))            # <= 2^25 complex128 elements (512 MB) per temporary
        return [(i, min(i + per, self.N)) for i in range(0, self.N, per)]

    def up(self, vec):
        v = np.asarray(vec)
        v = np.ascontiguousarray(v.astype(np.complex128 if np.iscomplexobj(v) else np.float64))
        return self.torch.from_numpy(v).to(self.dev)

    def factors(self, terms):
        return [tuple(self.up(v) for v in t) for t in terms]

    def spectra(self, terms, conj=False):
        """the 1-D transforms of every factor, in long double, rounded once to double (conj: of the inverse transform)"""
        import scipy.fft
        out = []
        for t in terms:
            f = [scipy.fft.fft(np.asarray(v, dtype=np.longdouble)) for v in t]
            assert f[0].dtype == np.clongdouble
            out.append(tuple(self.up((np.conj(v) if conj else v).astype(np.complex128)) for v in f))
        return out

    @staticmethod
    def outer(fac, i0, i1, nlast, scale=1.0):
        tot = None
        for a, b, c in fac:
            term = (a[i0:i1, None, None] * scale) * b[None, :, None] * c[None, None, :nlast]
            tot = term if tot is None else tot + term
        return tot

    def fill(self, view, fac, nlast, imag=None):
        """view[...] = outer product of the factors (+ i that of `imag`), formed in double, cast once"""
        for i0, i1 in self.chunks(nlast):
            w = self.outer(fac, i0, i1, nlast)
            if imag is not None:
                w = self.torch.complex(w, self.outer(imag, i0, i1, nlast))
            view[i0:i1].copy_(w)

    def compare(self, view, parts, nlast, scale=1.0):
        """Every element of `view` against sum_p coef_p outer(parts[p]) in double: max |err|, rms err, (rms, max) of the
        reference and of each of its parts."""
        t = self.torch

        def zero():
            return t.zeros((), dtype=t.float64, device=self.dev)

        def mod2(w):
            return (w.real ** 2 + w.imag ** 2) if w.is_complex() else w * w
        emax, esum, wsum, wmax = zero(), zero(), zero(), zero()
        pstat = [[zero(), zero()] for _ in parts]
        for i0, i1 in self.chunks(nlast):
            want = None
            for q, (coef, fac) in enumerate(parts):
                w = self.outer(fac, i0, i1, nlast, scale)
                m2 = mod2(w)
                pstat[q][0] += m2.sum()
                pstat[q][1] = t.maximum(pstat[q][1], m2.max())
                w = w * coef if coef != 1 else w
                want = w if want is None else want + w
            m2 = mod2(want)
            wsum += m2.sum()
            wmax = t.maximum(wmax, m2.max())
            d = view[i0:i1].to(t.complex128 if want.is_complex() else t.float64) - want
            e2 = mod2(d)
            esum += e2.sum()
            emax = t.maximum(emax, e2.max())
            del want, d, e2, m2, w
        n = float(self.N) ** 2 * nlast
        return dict(emax=float(emax.sqrt()), erms=float((esum / n).sqrt()), wrms=float((wsum / n).sqrt()),
                    wmax=float(wmax.sqrt()), parts=[(float((s / n).sqrt()), float(m.sqrt())) for s, m in pstat])


def _judge(rig, label, names, st, log, fails, extra_rms=0.0):
    """both bounds of one comparison; `names`: the case of every part of the reference (errors of the parts add)"""
    N, pr = rig.N, rig.precision
    bmax = sum(sn.max_bound(pr, N, nm, rms, mx) for nm, (rms, mx) in zip(names, st["parts"])) + REF_ERR * st["wmax"]
    brms = (sn.rms_bound(pr, N) + extra_rms + REF_ERR) * st["wrms"]
    line = "%-40s max %.3e (bound %.3e)  rms %.3e (bound %.3e)  max/rms(want) %.3e  rms/rms(want) %.3e" % (
        label, st["emax"], bmax, st["erms"], brms, st["emax"] / st["wrms"], st["erms"] / st["wrms"])
    log.append(line)
    print(line, flush=True)
    if not (st["emax"] <= bmax and st["erms"] <= brms):
        fails.append(line)


def _real_transforms(rig, cases, log, fails, nondestroying):
    from fastbox_amd.device import DeviceArray, HALF, REAL, _Buffer
    t = rig.torch
    N, nz = rig.N, rig.nz
    real, half = rig.new_real(), rig.new_half()
    hv = rig.half_view(half)
    eps = sn.EPS[rig.precision]
    for name in cases:
        terms = sn.case_terms(name, N)
        fac, spec = rig.factors(terms), rig.spectra(terms)
        tag = "%d %s %s " % (N, rig.precision, name)
        rig.fill(real, fac, N)
        rig.call("fb_fft_r2c", real.data_ptr(), half.data_ptr(), 0, rig.stream())
        _judge(rig, tag + "r2c", [name], rig.compare(hv, [(1, spec)], nz), log, fails)
        half.zero_()
        rig.fill(hv, spec, nz)
        if nondestroying:
            keep = half.clone()
            t.cuda.synchronize()
            wrapped = DeviceArray(rig.eng, HALF, _Buffer(half.data_ptr(), rig.eng.nbytes[HALF], None))
            out = rig.eng.fft_c2r(wrapped)                   # the engine's stream is the null stream, which is torch's
            rig.lib.call("fb_memcpy_d2d", real.data_ptr(), out.ptr, rig.eng.nbytes[REAL], rig.stream())
            t.cuda.synchronize()
            del out, wrapped
            _judge(rig, tag + "c2r keeping its input", [name], rig.compare(real, [(1, fac)], N), log, fails, extra_rms=eps)
            if not t.equal(keep, half):
                fails.append(tag + "c2r(destroy=False) changed its input")
            del keep
            rig.eng.release_idle_buffers()
        real.zero_()
        rig.call("fb_fft_c2r", half.data_ptr(), real.data_ptr(), 1.0 / float(N) ** 3, rig.stream())
        _judge(rig, tag + "c2r", [name], rig.compare(real, [(1, fac)], N), log, fails, extra_rms=eps)
    del real, half, hv


def _complex_transforms(rig, pairs, log, fails):
    t = rig.torch
    N = rig.N
    full = rig.new_full()
    fv = t.view_as_complex(full)
    for p, q in pairs:
        tp, tq = sn.case_terms(p, N), sn.case_terms(q, N)
        fp, fq = rig.factors(tp), rig.factors(tq)
        tag = "%d %s %s + i %s " % (N, rig.precision, p, q)
        for sign, conj, scale, what in ((-1, False, 1.0, "c2c forward"), (+1, True, 1.0 / float(N) ** 3, "c2c inverse")):
            rig.fill(fv, fp, N, imag=fq)
            rig.call("fb_fft_c2c", full.data_ptr(), sign, scale, rig.stream())
            sp, sq = rig.spectra(tp, conj), rig.spectra(tq, conj)
            _judge(rig, tag + what, [p, q], rig.compare(fv, [(1, sp), (1j, sq)], N, scale), log, fails)
    del full, fv


def _finish(log, fails):
    assert not fails, "%d of %d comparisons out of bounds:\n%s" % (len(fails), len(log), "\n".join(fails))


@pytest.mark.parametrize("N,precision", [(512, "f32"), (512, "f64"), (1024, "f32"), (1024, "f64")])
def test_transforms_against_separable_reference(N, precision):
    """r2c, c2r (destroying and not), c2c forward and inverse, all cases.  512^3 is the harness at a size other tests pin."""
    rig = _Rig(N, precision)
    log, fails = [], []
    try:
        _real_transforms(rig, sn.CASES, log, fails, nondestroying=True)
        _complex_transforms(rig, sn.complex_pairs(), log, fails)
    finally:
        rig.close()
    _finish(log, fails)


@pytest.mark.parametrize("variant", ["default", "rows64", "one_tile_per_workgroup"])
def test_transforms_at_2048_single_precision(variant):
    """r2c and c2r, all cases: with the plan's defaults (what bench.py times: 128-byte rows, resident schedule), with 64-byte rows,
    and with one workgroup per tile.  c2c (a 68.7 GB buffer, see the module docstring) with the defaults."""
    N = 2048
    assert N ** 3 * 8 + 3e9 < DEVICE_BYTES_BOUND
    rig = _Rig(N, "f32")
    log, fails = [], []
    try:
        if variant == "rows64":
            rig.eng.set_tile_rows(64)
        if variant == "one_tile_per_workgroup":
            rig.eng.set_pass_schedule(0, 0, 0)
        _real_transforms(rig, sn.CASES, log, fails, nondestroying=False)
        if variant == "default":
            gc.collect()
            rig.torch.cuda.empty_cache()
            _complex_transforms(rig, sn.complex_pairs(), log, fails)
    finally:
        rig.close()
    _finish(log, fails)


def test_transforms_at_2048_double_precision():
    """r2c and the destroying c2r, all cases: 68.7 GB + 69.8 GB + chunks, under three quarters of the device's memory."""
    N = 2048
    rig = _Rig(N, "f64")
    log, fails = [], []
    try:
        assert rig.eng.nbytes["real"] + rig.eng.nbytes["half"] + 3e9 < DEVICE_BYTES_BOUND
        _real_transforms(rig, sn.CASES, log, fails, nondestroying=False)
    finally:
        rig.close()
    _finish(log, fails)


# ---- generator ---------------------------------------------------------------------------------------------------------------
def _planes(N):
    H = N // 2
    rs = np.random.RandomState(N)
    return [0, 1, H - 1, H] + sorted(int(v) for v in rs.choice(np.arange(2, H - 1), size=4, replace=False))


def _host_amplitude(N, L, planes):
    """sqrt(nan_to_num(P(k)) boxfactor) on the planes, (N, N, len(planes)), from the mode numbers (the reference's expression
    for |k|), P(k) evaluated once per distinct |k|."""
    m = np.fft.fftfreq(N, 1.0 / N)
    k2 = ((m / L[0]) ** 2)[:, None, None] + ((m / L[1]) ** 2)[None, :, None] + ((m[planes] / L[2]) ** 2)[None, None, :]
    k = 2.0 * np.pi * np.sqrt(k2)
    uk, inv = np.unique(k, return_inverse=True)
    with np.errstate(all="ignore"):
        pk = np.nan_to_num(standin.pk_fn(standin.cosmology(), 1.0)(uk))
    boxfactor = float(N) ** 6 / (L[0] * L[1] * L[2])
    return np.sqrt(pk * boxfactor)[inv.reshape(k.shape)]


def _gather(rig, half, planes):
    idx = rig.torch.as_tensor(planes, device=rig.dev)
    return rig.half_view(half).index_select(2, idx).to(rig.torch.complex128).cpu().numpy()


@pytest.mark.parametrize("N,precision,L", [(1024, "f32", 1e3), (1024, "f64", 1e3), (1024, "f32", (1e3, 7e2, 1.3e3)),
                                           (2048, "f32", 2e3)])
def test_generator_against_host_model(N, precision, L):
    from fastbox_amd import CosmoBox, default_cosmo, rng
    H = N // 2
    planes = _planes(N)
    assert len(set(planes)) == 8 and {0, 1, H - 1, H} <= set(planes)
    box = CosmoBox(cosmo=default_cosmo, box_scale=L, nsamp=N, realise_now=False, precision=precision, rng="device", seed=SEED)
    box._set_amplitude(1.0, False)
    amp = _host_amplitude(N, (box.Lx, box.Ly, box.Lz), planes)
    # (c) the corner of the cube is in the compared set with a non-zero amplitude; the k = 0 mode has none
    assert amp[H, H, planes.index(H)] > 0.0 and amp[0, 0, 0] == 0.0
    if N == 2048:
        ix, iy = np.arange(N, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
        idx = ((ix % H) * N + iy) * (H + 1) + 1                          # the plane k_z = 1 (no mirrored draws on it)
        assert 1 in planes and (idx >= 2 ** 31).sum() >= 2 * (N - 2) and idx.max() < 2 ** 32
    rig = _Rig(N, precision, engine=box.engine)
    tol = GEN_TOL[precision]
    log, fails = [], []

    def note(line, ok):
        log.append(line)
        print(line, flush=True)
        if not ok:
            fails.append(line)
    try:
        half, real = rig.new_half(), rig.new_real()
        for r in (0, 1):
            z = rng.half_spectrum_noise(N, SEED, r, np.float32 if precision == "f32" else np.float64, planes=planes)
            want = z * amp
            half.zero_()
            rig.call("fb_colour_device", SEED, r, half.data_ptr(), rig.stream())
            got = _gather(rig, half, planes)
            ratio = np.abs(got - want) / (amp * (1.0 + np.abs(z)) + 1e-300)
            for q, iz in enumerate(planes):
                worst = float(ratio[:, :, q].max())
                note("%d %s L=%s r=%d kz=%d (a) colour_device: max |err| / (amp (1 + |z|)) %.3e (bound %.1e)" % (
                    N, precision, L, r, iz, worst, tol), worst <= tol)
            half.zero_()
            rig.call("fb_realise_density_begin", SEED, r, half.data_ptr(), rig.stream())
            rig.call("fb_realise_density_finish", half.data_ptr(), real.data_ptr(), rig.stream())
            half.zero_()
            rig.call("fb_fft_r2c", real.data_ptr(), half.data_ptr(), 0, rig.stream())
            got = _gather(rig, half, planes)
            for q, iz in enumerate(planes):
                scale = np.sqrt(np.mean(np.abs(want[:, :, q]) ** 2)) * np.sqrt(np.log2(float(N) ** 3) / 27.0)
                worst = float(np.abs(got[:, :, q] - want[:, :, q]).max() / scale)
                note("%d %s L=%s r=%d kz=%d (b) fused route + r2c: max |err| / (rms |z amp| sqrt(levels / 27)) %.3e (bound %.1e)" % (
                    N, precision, L, r, iz, worst, tol), worst <= tol)
            del z, want, got, ratio
        del half, real
    finally:
        rig.close()
        del box
        gc.collect()
    _finish(log, fails)
