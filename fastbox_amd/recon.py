"""
Density-field (BAO) reconstruction and mesh readout on the device (Eisenstein et al. 2007; Padmanabhan et al. 2012; Burden
et al. 2014): what nbodykit and pyrecon provide to the host pipelines.  Definition, conventions and limits: DESIGN.md section 4;
numpy statement: tests/recon_numpy.py; kernels: csrc/fb_recon.hip.

    rec = box.reconstruct(particles, smoothing=10., bias=1., f=0.5)        # Reconstruction
    rec.delta_rec                                                           # real DeviceArray: D / nbar_D - S / nbar_S
    xi = recon.reconstructed_xi(box, rec, edges)                            # (DD - 2 DS + SS) / RR
    v = box.readout([vx, vy, vz], halos)                                    # fields at catalogue positions, (n, 3) on the device
    randoms = box.uniform_catalogue(10 ** 6)

The line of sight is z.  Random positions are Philox stream 10, reproduced by ``fastbox_amd.rng.recon_uniforms``.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, HALF, REAL
from .halos import HaloCatalogue, WINDOWS, _next_realisation, pair_counts

CONVENTIONS = ("sym", "iso")
N_MAX = 2 ** 31 - 2


class DeviceValues(DeviceBuffer):
    """fp64 values per particle on the device, shape (n,) or (n, k); ``np.asarray(v)`` is the host copy."""

    def __init__(self, engine, buf, shape):
        DeviceBuffer.__init__(self, engine, buf, shape, np.float64)

    def __repr__(self):
        return "DeviceValues(shape=%s)" % (self.shape,)


class Reconstruction(object):
    """The result of ``CosmoBox.reconstruct``: ``delta_rec`` (real DeviceArray, D / nbar_D - S / nbar_S), ``data`` and
    ``randoms`` (the shifted catalogues, HaloCatalogues that ``pair_counts``, ``paint_catalogue`` and ``grid_catalogue`` take),
    ``displacement`` (three real DeviceArrays Psi_x, Psi_y, Psi_z in Mpc, or None unless asked for), ``n_data``, ``n_random``,
    ``smoothing`` (Mpc), ``bias``, ``f``, ``convention`` and ``window``."""

    def __init__(self, delta_rec, data, randoms, displacement, smoothing, bias, f, convention, window):
        self.delta_rec, self.data, self.randoms, self.displacement = delta_rec, data, randoms, displacement
        self.n_data, self.n_random = data.n, randoms.n
        self.smoothing, self.bias, self.f, self.convention, self.window = float(smoothing), float(bias), float(f), convention, window

    def __repr__(self):
        return "Reconstruction(%d data, %d randoms, R = %g Mpc, b = %g, f = %g, '%s')" % (
            self.n_data, self.n_random, self.smoothing, self.bias, self.f, self.convention)


# ---------------------------------------------------------------------- arguments
def _box_sides(box):
    return (float(box.Lx), float(box.Ly), float(box.Lz))


def _window(window):
    if window not in WINDOWS:
        raise ValueError("window must be one of %s" % sorted(WINDOWS))
    return WINDOWS[window]


def _check_range(lohi, L, name):
    """finite and |x| < 2^52 L on every axis (beyond it x - L floor(x / L) is off by units of ulp(x) >= L)"""
    for a in range(3):
        lo, hi = lohi[2 * a], lohi[2 * a + 1]
        if not (np.isfinite(lo) and np.isfinite(hi)) or max(abs(lo), abs(hi)) >= 2. ** 52 * L[a]:
            raise ValueError("%s: a position is not finite, or too large to wrap into the box" % name)


def _positions(box, x, name, keep):
    """(n, device pointer or None) of a catalogue argument -- a HaloCatalogue of this box (ColaParticles, FoFHalos, SOHalos)
    or a host (n, 3) array -- checked as find_halos checks its particles."""
    eng, L = box.engine, _box_sides(box)
    if isinstance(x, HaloCatalogue):
        if x.engine is not eng:
            raise ValueError("%s: a catalogue of this box" % name)
        if x.n > N_MAX:
            raise ValueError("%s: at most 2^31 - 2 particles" % name)
        if x.n:
            lohi = (ctypes.c_double * 6)()
            _lib.call("fb_position_range", eng._plan, x.ptr, x.n, lohi, eng.stream)
            _check_range(list(lohi), L, name)
        keep.append(x)
        return x.n, x.ptr
    if isinstance(x, (str, bytes)) or np.iscomplexobj(x):
        raise TypeError("%s: a catalogue of this box or a real (n, 3) array" % name)
    p = np.ascontiguousarray(x, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("%s: an (n, 3) array" % name)
    if p.shape[0] > N_MAX:
        raise ValueError("%s: at most 2^31 - 2 particles" % name)
    if p.shape[0]:
        _check_range([f(p[:, a]) for a in range(3) for f in (np.min, np.max)], L, name)
        keep.append(eng.upload_raw(p))
        return p.shape[0], keep[-1].ptr
    return 0, None


def _real_field(box, a, name, keep):
    """The device pointer of one real field: a real DeviceArray of this box or a host (N, N, N) real array."""
    eng = box.engine
    if isinstance(a, DeviceArray):
        if a.engine is not eng:
            raise ValueError("%s: a field of this box" % name)
        if a.kind != REAL or a._as_complex:
            raise TypeError("%s: a real field, not a complex one or a spectrum" % name)
        keep.append(a)
        return a
    h = np.asarray(a)
    if np.iscomplexobj(h):
        raise TypeError("%s: a real field, not a complex one" % name)
    d = eng.upload(h, REAL)
    keep.append(d)
    return d


def _pack(box, fields, name, keep):
    """(pointer, k, single) of one to three real fields as one T[k][N^3] block."""
    eng = box.engine
    single = isinstance(fields, DeviceArray) or (isinstance(fields, np.ndarray) and fields.ndim == 3)
    fl = [fields] if single else list(fields)
    if not 1 <= len(fl) <= 3:
        raise ValueError("%s: one to three fields" % name)
    dev = [_real_field(box, a, name, keep) for a in fl]
    if len(dev) == 1:
        return dev[0].ptr, 1, single
    nb = eng.nbytes[REAL]
    blk = eng._alloc_bytes(len(dev) * nb)
    keep.append(blk)
    for c, d in enumerate(dev):
        _lib.call("fb_memcpy_d2d", blk.ptr + c * nb, d.ptr, nb, eng.stream)
    return blk.ptr, len(dev), single


def _params(smoothing, bias, f):
    smoothing, bias, f = float(smoothing), float(bias), float(f)
    if not (np.isfinite(smoothing) and smoothing > 0.):
        raise ValueError("smoothing: a positive length in Mpc")
    if not (np.isfinite(bias) and bias > 0.):
        raise ValueError("bias: a positive number")
    if not (np.isfinite(f) and f >= 0.):
        raise ValueError("f: a growth rate >= 0")
    return smoothing, bias, f


# ---------------------------------------------------------------------- stages
def readout(box, field, positions, window='cic'):
    """CosmoBox.readout: see there."""
    eng = box.engine
    w = _window(window)
    keep = []
    fptr, k, single = _pack(box, field, "field", keep)
    n, pptr = _positions(box, positions, "positions", keep)
    out = eng._alloc_bytes(8 * n * k) if n else None
    _lib.call("fb_mesh_readout", eng._plan, fptr, k, pptr, n, w, out.ptr if n else None, eng.stream)
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    return DeviceValues(eng, out, (n,) if single else (n, k))


def uniform_catalogue(box, n, seed=None, realisation=None):
    """CosmoBox.uniform_catalogue: see there."""
    eng = box.engine
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= N_MAX:
        raise ValueError("n: an integer between 0 and 2^31 - 2")
    n = int(n)
    if realisation is None:             # the box's next draw, or draw 0 of a seed given for this call
        realisation = _next_realisation(box) if seed is None else 0
    seed, real = (box.seed if seed is None else int(seed)), int(realisation)
    if n == 0:
        return HaloCatalogue(eng, None, 0)
    buf = eng._alloc_bytes(24 * n)
    _lib.call("fb_uniform_positions", eng._plan, seed & (2 ** 64 - 1), real & (2 ** 64 - 1), n, buf.ptr, eng.stream)
    cat = HaloCatalogue(eng, buf, n)
    cat.seed, cat.realisation = seed, real
    return cat


def grid_catalogue_nodes(box):
    """One particle on each mesh node, C order: the randoms without shot noise (``randoms='grid'``)."""
    eng, n = box.engine, int(box.N) ** 3
    if n > N_MAX:
        raise ValueError("randoms='grid': at most 2^31 - 2 nodes")
    buf = eng._alloc_bytes(24 * n)
    _lib.call("fb_grid_positions", eng._plan, buf.ptr, eng.stream)
    return HaloCatalogue(eng, buf, n)


def density_contrast(box, positions, window='cic'):
    """delta = n / nbar - 1 of a catalogue on the box's grid: ``paint_catalogue`` times N^3 / n, minus 1; a real DeviceArray.
    The density ``reconstruct`` starts from when no ``delta`` is given."""
    keep = []
    n, pptr = _positions(box, positions, "positions", keep)
    if not n:
        raise ValueError("positions: at least one particle")
    out = _density_of(box, pptr, n, _window(window))
    box.engine.sync()                   # host arrays behind the uploads must outlive the copies
    return out


def _displacement_block(box, delta, smoothing, bias, f, keep):
    """Psi as one T[3][N^3] block from a real field, or a half spectrum, of this box."""
    eng = box.engine
    if isinstance(delta, DeviceArray) and delta.kind == HALF and delta.engine is eng:
        half = delta
    else:
        half = eng.fft_r2c(_real_field(box, delta, "delta", keep))
    keep.append(half)
    work = eng._alloc_bytes(3 * eng.nbytes[HALF])
    psi = eng._alloc_bytes(3 * eng.nbytes[REAL])
    _lib.call("fb_recon_displacement", eng._plan, half.ptr, work.ptr, psi.ptr, smoothing, bias, f / bias, eng.stream)
    return psi


def _split(box, psi):
    eng, nb = box.engine, box.engine.nbytes[REAL]
    out = []
    for c in range(3):
        d = eng.empty(REAL)
        _lib.call("fb_memcpy_d2d", d.ptr, psi.ptr + c * nb, nb, eng.stream)
        out.append(d)
    return tuple(out)


def displacement(box, delta, smoothing=10., bias=1., f=0.):
    """(Psi_x, Psi_y, Psi_z), real DeviceArrays in Mpc: the inverse transforms of i k_a delta(k) exp(-k^2 R^2 / 2) / (b (k^2 +
    beta k_z^2)), beta = f / b.  ``delta``: a real field of this box (DeviceArray or host array), or
    its half spectrum (``box.engine.fft_r2c``)."""
    smoothing, bias, f = _params(smoothing, bias, f)
    keep = []
    return _split(box, _displacement_block(box, delta, smoothing, bias, f, keep))


def displace_catalogue(box, displacement_fields, positions, window='cic', scale=1., scale_z=0., inplace=False):
    """A catalogue moved by a field on the device: wrap(x - scale Psi(x) - scale_z Psi_z(x) z^), Psi read off the three fields at
    each particle through ``window``.  ``positions``: a HaloCatalogue of this box or a host (n, 3) array; ``inplace`` (a
    HaloCatalogue only) overwrites it.  Returns a HaloCatalogue."""
    eng = box.engine
    w = _window(window)
    keep = []
    fptr, k, _ = _pack(box, displacement_fields, "displacement_fields", keep)
    if k != 3:
        raise ValueError("displacement_fields: three fields (x, y, z)")
    n, pptr = _positions(box, positions, "positions", keep)
    out = _shift(box, fptr, n, pptr, w, float(scale), float(scale_z),
                 positions if inplace and isinstance(positions, HaloCatalogue) else None)
    eng.sync()
    return out


def _shift(box, psi_ptr, n, pptr, w, scale, scale_z, into):
    eng = box.engine
    if n == 0:
        return HaloCatalogue(eng, None, 0)
    out = into if into is not None else HaloCatalogue(eng, eng._alloc_bytes(24 * n), n)
    _lib.call("fb_recon_shift", eng._plan, psi_ptr, pptr, n, w, scale, scale_z, out.ptr, eng.stream)
    out._host = None
    return out


def reconstruct(box, data, randoms=None, smoothing=10., bias=1., f=0., convention='sym', window='cic', delta=None, seed=None,
                return_displacement=False):
    """CosmoBox.reconstruct: see there."""
    eng, N = box.engine, int(box.N)
    smoothing, bias, f = _params(smoothing, bias, f)
    if convention not in CONVENTIONS:
        raise ValueError("convention must be 'sym' (RecSym) or 'iso' (RecIso)")
    w = _window(window)
    keep = []
    if isinstance(randoms, str) and randoms != 'grid':
        raise ValueError("randoms: None, a number of draws, 'grid', a catalogue of this box or an (n, 3) array")
    nd, dptr = _positions(box, data, "data", keep)
    if nd == 0:
        raise ValueError("data: at least one particle")
    grid = isinstance(randoms, str)
    drawn = randoms is None or (isinstance(randoms, (int, np.integer)) and not isinstance(randoms, bool))
    if randoms is None:
        nr = 4 * nd
    elif grid:
        nr = N ** 3
    elif drawn:
        nr = int(randoms)
    else:
        nr, rptr = _positions(box, randoms, "randoms", keep)
    if not 1 <= nr <= N_MAX:
        raise ValueError("randoms: between 1 and 2^31 - 2 particles")
    eng.need_memory(int(eng.lib.fb_recon_work_bytes(eng._plan, nd, nr)),
                    "reconstruct: %d data and %d randoms on a %d^3 grid take" % (nd, nr, N))
    own = None                          # randoms made here are shifted in place
    if grid or drawn:
        own = grid_catalogue_nodes(box) if grid else uniform_catalogue(box, nr, seed=seed, realisation=0)
        rptr = own.ptr
    if delta is None:
        delta = _density_of(box, dptr, nd, w)
    psi = _displacement_block(box, delta, smoothing, bias, f, keep)
    sdata = _shift(box, psi.ptr, nd, dptr, w, 1., f, None)
    srand = _shift(box, psi.ptr, nr, rptr, w, 1., f if convention == 'sym' else 0., own)
    D, S = eng.empty(REAL), eng.empty(REAL)
    _lib.call("fb_paint", eng._plan, sdata.ptr, None, nd, w, D.ptr, eng.stream)
    _lib.call("fb_paint", eng._plan, srand.ptr, None, nr, w, S.ptr, eng.stream)
    n3 = float(N) ** 3
    rec = eng.axpby(D, S, n3 / nd, -(n3 / nr), 0.)
    disp = _split(box, psi) if return_displacement else None
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    return Reconstruction(rec, sdata, srand, disp, smoothing, bias, f, convention, window)


def _density_of(box, pptr, n, w):
    """density_contrast of positions already on the device"""
    eng = box.engine
    mesh = eng.empty(REAL)
    _lib.call("fb_paint", eng._plan, pptr, None, n, w, mesh.ptr, eng.stream)
    return eng.axpby(mesh, None, float(box.N) ** 3 / n, 0., -1.)


def reconstructed_xi(box, rec, edges=None, mode='1d', Nmu=10, pimax=None, poles=None):
    """The correlation function of a ``Reconstruction`` in the Landy-Szalay form (DD - 2 DS + SS) / RR from three
    ``pair_counts`` calls on the shifted data D and the shifted randoms S: DD and SS are auto-counts normalised by
    n (n - 1), DS the cross-count normalised by n_D n_S, and RR the analytic V_bin / V_box of the periodic box that
    ``PairCounts.rr`` holds (per pair).  Host arithmetic on the returned counts only.  Returns (r, xi): the bin midpoints and
    xi of the counts' shape; with ``poles`` ('2d') xi is a dict l -> xi_l(r)."""
    dd = pair_counts(box, rec.data, None, edges=edges, mode=mode, Nmu=Nmu, pimax=pimax)
    ds = pair_counts(box, rec.data, rec.randoms, edges=edges, mode=mode, Nmu=Nmu, pimax=pimax)
    ss = pair_counts(box, rec.randoms, None, edges=edges, mode=mode, Nmu=Nmu, pimax=pimax)
    with np.errstate(divide='ignore', invalid='ignore'):
        xi = dd.npairs / dd.rr - 2. * (ds.npairs / ds.rr) + ss.npairs / ss.rr       # each term is count / (pairs V_bin / V_box)
    if poles is not None:
        from .halos import _LEGENDRE, _check_pair_poles
        if mode != '2d':
            raise ValueError("poles: with mode='2d' only")
        mu = 0.5 * (dd.mu_edges[1:] + dd.mu_edges[:-1])
        dmu = np.diff(dd.mu_edges)
        return dd.r, {l: (2 * l + 1) * np.sum(xi * (_LEGENDRE[l](mu) * dmu)[None, :], axis=1) for l in _check_pair_poles(poles)}
    return dd.r, xi
