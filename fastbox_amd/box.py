"""
``CosmoBox`` -- drop-in for the density-field hot path of ``fastbox.box.CosmoBox``
(philbull/FastBox, fastbox/box.py) with the arithmetic running as HIP kernels
on an MI355X behind libfastbox_hip.so.

Same constructor, method names, argument order, defaults and exceptions as the
reference; fields are returned as ``DeviceArray`` objects that stay in HBM and
turn into float64 / complex128 ndarrays when numpy touches them.  Additive,
reference-preserving keyword arguments: ``precision`` ('f32' storage with fp64
bin sums, or 'f64'), ``rng`` ('numpy' = the reference's legacy global stream,
drawn on the host and uploaded -- same seed, same field; 'device' = on-device
counter-based Philox4x32-10 RNG for throughput, reproducible on the host with
``fastbox_amd.rng``), ``seed``, ``device``, ``stream``.

No CPU fallback exists: without the HIP library or a GPU every compute method
raises.
"""
import weakref

import numpy as np

from . import hostgeom

from . import cosmology as _builtin_cosmology
from . import device as _dev
from ._lib import FB_FILT_TABLE, FB_FILT_TOPHAT
from .device import DeviceArray, Engine, FULL, HALF, REAL
from .transfer import DeviceFilter

try:                                        # the reference's provider, if present
    import pyccl as _ccl
except Exception:                           # not installed in this image
    _ccl = _builtin_cosmology

# Speed of light (m/s)
C = 299792458.

default_cosmo = dict(Omega_c=0.25, Omega_b=0.05, h=0.7, n_s=0.95, sigma8=0.8,
                     transfer_function='eisenstein_hu')

try:
    from scipy.integrate import simpson as _simpson
except Exception:                           # pragma: no cover
    from scipy.integrate import simps as _simpson


def _finish_bins(cnt, s1, s2, boxfactor, eps=0.):
    """(mean, std/sqrt(n)) per bin from (count, sum |dk|^2, sum |dk|^4), bin 0 dropped
    (box.py:761-768); see hostgeom.finish_bins."""
    return hostgeom.finish_bins(cnt, s1, s2, boxfactor, eps)


def _eps_of(engine):
    """rounding unit of the plan's |delta_k|^2 values: the precision floor of the variance form"""
    return 2. ** -23 if engine.precision == "f32" else 2. ** -52


class _Ready(object):
    def __init__(self, out):
        self._out = out

    def result(self):
        return self._out


class PendingSpectrum(object):
    """Handle on a power spectrum whose bin sums are still being computed on the device."""

    def __init__(self, engine, res, nbins, kc, boxfactor, ln_voxels, keepalive, redo=None):
        self._eng, self._res, self._nb, self._kc, self._bf = engine, res, nbins, kc, boxfactor
        self._lnv, self._keep, self._out = ln_voxels, keepalive, None
        self._cnt = engine.bin_counts()
        self._raw = None                       # the device record, delivered by the engine's batched fetch
        self._redo = redo                      # log-normal: () -> (s1, s2, esum) with the exact shift (see result)
        self.repeated = False
        engine.register_waiter(res, self)

    def _in_range(self, s1, s2, esum):
        return hostgeom.lognormal_sums_in_range(self._cnt, s1, s2, esum)

    @staticmethod
    def _finish_batch(owners):
        """The host arithmetic of `result()` for every record of one fetch at once (same numpy expressions, broadcast over
        the records: identical numbers).  Records whose log-normal sums are out of range are left to `result()`, which
        repeats the step."""
        groups = {}
        for o in owners:
            if type(o) is PendingSpectrum and o._out is None and o._raw is not None:
                groups.setdefault((o._nb, id(o._cnt), o._lnv, o._bf, _eps_of(o._eng)), []).append(o)
        for (nb, _, lnv, bf, eps), grp in groups.items():
            if len(grp) < 2:
                continue
            R = np.stack([o._raw for o in grp])
            s1, s2, esum = R[:, 0:2 * nb:2], R[:, 1:2 * nb:2], R[:, 2 * nb]
            cnt = grp[0]._cnt
            good = np.ones(len(grp), dtype=bool)
            with np.errstate(all="ignore"):
                if lnv:
                    good = hostgeom.lognormal_sums_in_range_many(cnt, s1, s2, esum)
                    mean = esum / lnv
                    s1, s2 = hostgeom.lognormal_rescale(s1, s2, mean)
                vals, std = hostgeom.finish_bins_many(cnt, s1, s2, bf, eps)
            for i, o in enumerate(grp):
                if good[i]:
                    o._out = (o._kc, vals[i].copy(), std[i].copy())
                    o._res = o._keep = o._redo = None

    def result(self):
        if self._out is None:
            s1, s2, esum = self._eng.fetch_results(self._res, self._nb, owner=self)
            if self._lnv:                      # transform of exp(d - shift): rescale to exp(d)/mean - 1
                if not self._in_range(s1, s2, esum):
                    # the shift was taken from the field's variance (hostgeom.lognormal_shift) and this realisation's
                    # largest values lie outside what that allows for: once more, with the shift from its maximum
                    if self._redo is None:
                        raise FloatingPointError("log-normal P(k): the exponentials left the plan's floating-point "
                                                 "range (sum = %r)" % (esum,))
                    s1, s2, esum = self._redo()
                    self.repeated = True
                    if not self._in_range(s1, s2, esum):
                        raise FloatingPointError("log-normal P(k): non-finite bin sums (sum of exponentials %r); "
                                                 "is the field finite?" % (esum,))
                mean = esum / self._lnv
                s1, s2 = hostgeom.lognormal_rescale(s1, s2, mean)
            self._out = (self._kc,) + _finish_bins(self._cnt, s1, s2, self._bf, _eps_of(self._eng))
            self._res = self._keep = self._redo = None
        return self._out


class LognormalField(DeviceArray):
    """exp(d)/<exp(d)> - 1 of a device field, materialised on first read."""

    def __init__(self, engine, source):
        DeviceArray.__init__(self, engine, REAL, None)
        self.source = source

    @property
    def materialised(self):
        return self._buf is not None

    @property
    def ptr(self):
        if self._buf is None:
            out, _ = self.engine.lognormal(self.source)
            self._buf = out._buf
        return self._buf.ptr


class LazySpectrum(DeviceArray):
    """A k-space field computed by `make()` on first use (e.g. one velocity component: callers of the
    reference usually transform only v_z, box.py:285 returns all three)."""

    def __init__(self, engine, kind, make, recipe=None, source_real=None):
        DeviceArray.__init__(self, engine, kind, None)
        self._make = make
        self.recipe = recipe      # (amp_key, seed, realisation, comp, fac) of a device-RNG velocity component
        self.source_real = source_real    # to_k(field): the real field this is the (pending) transform of

    @property
    def materialised(self):
        return self._buf is not None

    @property
    def ptr(self):
        if self._buf is None:
            self._buf = self._make()._buf
            self._make = None
        return self._buf.ptr


class FilteredField(DeviceArray):
    """ifftn(field_k * T(k_perp, k_par)) for a Hermitian device spectrum and a k_par-even ``DeviceFilter``
    (apply_transfer_fn, box.py:356-381), formed when it is first read.  ``binned_power_spectrum`` of it
    (or of its ``.real``) needs no transform of its own: it bins |field_k T|^2 from ``field_k``; when
    ``field_k`` is itself a pending ``CosmoBox.to_k(field)``, the multiply and the binning happen inside the last (x)
    pass of that forward transform, which also takes the inverse transform of each x line it has filtered -- reading
    the field afterwards costs the y and z passes only."""

    def __init__(self, engine, spectrum, filt, as_complex=True, parent=None):
        DeviceArray.__init__(self, engine, REAL, None, as_complex)
        self.spectrum, self.filter, self._parent = spectrum, filt, parent
        self._x_done = None              # field_k * T with its x lines already transformed back, once a fused P(k) has
                                         # produced it (see ptr)

    def _root(self):
        return self if self._parent is None else self._parent._root()

    @property
    def materialised(self):
        return self._buf is not None

    @property
    def ptr(self):
        if self._buf is None:
            root = self._root()
            if root is not self:
                root.ptr
                self._buf = root._buf
            elif self._x_done is not None:
                # the fused P(k) pass took the inverse x transform of every line it filtered: y and z remain
                self._buf = self.engine.fft_c2r_yz(self._x_done)._buf
                self._x_done = None
            else:
                dk = self.engine.apply_filter(self.spectrum, self.filter.kind, self.filter.params)
                self._buf = self.engine.fft_c2r(dk, destroy=True)._buf
        return self._buf.ptr

    @property
    def real(self):
        return FilteredField(self.engine, self.spectrum, self.filter, as_complex=False, parent=self)


class PendingDensity(DeviceArray):
    """delta_x of a device-RNG realisation whose last (z) FFT pass has not run yet.  Reading it
    runs that pass; ``binned_power_spectrum(delta_x=...)`` of it (or of its log-normal) instead
    fuses the pass with the power spectrum's first one, and fills in delta_x on the way."""

    def __init__(self, engine, pending_half, generator=None, regenerate=None, sigma2=None):
        DeviceArray.__init__(self, engine, REAL, None)
        self.sigma2 = sigma2            # variance of the distribution the field was drawn from (log-normal shift)
        self._pending = pending_half
        self.generator = generator      # (amp_key, seed, realisation): enough to regenerate delta_k
        self._regenerate = regenerate   # () -> real DeviceArray of the same realisation (counter-based generator)

    @property
    def materialised(self):
        return self._buf is not None

    def _adopt(self, real):
        self._buf, self._pending = real._buf, None

    @property
    def ptr(self):
        if self._buf is None:
            if self._pending is not None:
                self._adopt(self.engine.realise_finish(self._pending))
            else:
                # the pending spectrum went into a power spectrum that was asked not to keep the field
                # (binned_power_spectrum(..., keep_field=False)): draw the same realisation again
                self._adopt(self._regenerate())
        return self._buf.ptr


class RedshiftSpaceField(DeviceArray):
    """``redshift_space_density`` of two device-generator realisations (density, v_z) whose last FFT passes have not run
    yet.  Reading it finishes both and runs the remap kernel; asking for the power spectrum of its transform -- directly,
    or through ``apply_transfer_fn(to_k(...))`` -- instead runs ONE z pass per line of sight that finishes both inverse
    transforms, remaps and starts the forward transform (``Engine.power_redshift_space``): v_z in real space and this
    field itself are then never written.  The numbers are the same bit for bit."""

    def __init__(self, engine, delta, vz, args):
        DeviceArray.__init__(self, engine, REAL, None)
        self.delta, self.vz, self.args = delta, vz, args      # args = (Hz, sigma_nl, seed, method)

    @property
    def materialised(self):
        return self._buf is not None

    def fusable(self):
        return self._buf is None and self.delta is not self.vz and all(
            isinstance(f, PendingDensity) and not f.materialised and f._pending is not None for f in (self.delta, self.vz))

    def consume(self, filt=None, field=False):
        """The fused pass: (results buffer, work half spectrum); delta_x is filled in, v_z's pending spectrum is gone
        (reading v_z later draws it again)."""
        Hz, sigma_nl, seed, method = self.args
        res, real, work = self.engine.power_redshift_space(self.delta._pending, self.vz._pending, Hz, sigma_nl, seed, method,
                                                           filt=filt, field=field)
        self.delta._adopt(real)
        self.vz._pending = None
        return res, work

    @property
    def ptr(self):
        if self._buf is None:
            Hz, sigma_nl, seed, method = self.args
            self._buf = self.engine.redshift_space(self.delta, self.vz, Hz, sigma_nl, None, seed, method)._buf
        return self._buf.ptr


class CosmoBox(object):

    def __init__(self, cosmo, box_scale=1e3, nsamp=32, redshift=0.,
                 line_freq=1420.405752, realise_now=True,
                 precision="f32", rng="numpy", seed=0, device=0, stream=None):
        # box.py:61-64
        if isinstance(cosmo, dict):
            cosmo = _ccl.Cosmology(**cosmo)
        if not isinstance(cosmo, _ccl.Cosmology):
            raise TypeError("`cosmo` must be a CCL Cosmology object or dict.")
        self.cosmo = cosmo
        self.N = nsamp
        self.redshift = redshift
        self.scale_factor = 1. / (1. + redshift)
        self.line_freq = line_freq

        # grid including both end points, box.py:76-89
        if isinstance(box_scale, tuple):
            assert len(box_scale) == 3, "Must specify scale of x, y, z dimensions"
            self.x, self.y, self.z = [np.linspace(-0.5 * s, 0.5 * s, nsamp) for s in box_scale]
        else:
            self.x = self.y = self.z = np.linspace(-0.5 * box_scale, 0.5 * box_scale, nsamp)
        self.Lx = self.x[-1] - self.x[0]
        self.Ly = self.y[-1] - self.y[0]
        self.Lz = self.z[-1] - self.z[0]
        self.boxfactor = (self.N ** 6.) / (self.Lx * self.Ly * self.Lz)      # box.py:94
        self.kmin = 2. * np.pi / np.max([self.Lx, self.Ly, self.Lz])          # box.py:100
        self.kmax = 2. * np.pi * np.sqrt(3.) * self.N / np.min([self.Lx, self.Ly, self.Lz])

        if rng in ("threefry", "philox"):          # historical spellings of the device generator
            rng = "device"
        if rng not in ("numpy", "device"):
            raise ValueError("rng must be 'numpy' or 'device'")
        self.rng, self.seed, self._realisation = rng, int(seed), 0
        # grids that are not powers of two (round 4: even, prime factors 2, 3, 5, up to 1024 -- numpy's FFT takes any nsamp,
        # box.py:25-26): the library's plain FFT passes; nothing is fused into them, so such a box takes the step-by-step
        # routes a non-cubic box takes (exact |k| per mode instead of shell tables, stored spectra)
        self._plain = (self.N & (self.N - 1)) != 0
        self._cubic = (self.Lx == self.Ly == self.Lz) and not self._plain
        self._grids = None
        self._amp_key = None
        self._bin_cache = {}
        self._delta_k = None
        self.lognormal_repeats = 0        # fused log-normal spectra formed a second time with the exact shift
        self.set_fft_sample_spacing()
        self.engine = Engine(self.N, (self.Lx, self.Ly, self.Lz), self._axis2, self._ksc, self._kpar, self.z,
                             precision=precision, device=device, stream=stream)

        if realise_now:                                                       # box.py:104-107
            self.realise_density()
            self.realise_velocity()
            self.realise_potential()

    # ------------------------------------------------------------------ k grids
    def set_fft_sample_spacing(self):
        """1-D tables behind |k|, k_perp, k_par (box.py:119-127, 254-256, 374-375).  The
        (N,N,N) arrays Kx, Ky, Kz, k of the reference are never built on the device; the
        attributes of the same name materialise them on the host on first access."""
        N = self.N
        m = hostgeom.mode_numbers(N)        # the reference's own numbering, index-as-value quirk at non-powers of two included
        self._modes = m
        L = (self.Lx, self.Ly, self.Lz)
        self._axis2 = np.concatenate([(m / l) ** 2. for l in L])
        self._ksc = np.concatenate([m * (2. * np.pi / l) for l in L])
        self._kpar = 2. * np.pi * m / self.Lz
        self._grids = None

    def _host_grids(self):
        if self._grids is None:
            N, m = self.N, self._modes
            ones = np.ones((N, N, N))
            Kx, Ky, Kz = m[:, None, None] * ones, m[None, :, None] * ones, m[None, None, :] * ones
            k = 2. * np.pi * np.sqrt((Kx / self.Lx) ** 2. + (Ky / self.Ly) ** 2. + (Kz / self.Lz) ** 2.)
            self._grids = (Kx, Ky, Kz, k)
        return self._grids

    Kx = property(lambda self: self._host_grids()[0])
    Ky = property(lambda self: self._host_grids()[1])
    Kz = property(lambda self: self._host_grids()[2])
    k = property(lambda self: self._host_grids()[3])

    # --------------------------------------------------------------- conversions
    def _as_real(self, a):
        if isinstance(a, DeviceArray):
            if a.kind != REAL:
                raise TypeError("expected a real-space field")
            return a
        a = np.asarray(a)
        if np.iscomplexobj(a):
            a = a.real
        return self.engine.upload(a, REAL)

    def _as_spectrum(self, a):
        """DeviceArray half/full, or a host complex (N,N,N) array uploaded as 'full'."""
        if isinstance(a, DeviceArray):
            if a.kind == REAL:
                raise TypeError("expected a Fourier-space field")
            return a
        return self.engine.upload(np.asarray(a), FULL)

    @property
    def delta_k(self):
        """fftn(delta_x) (box.py:193), computed on first use after a realisation."""
        if self._delta_k is None:
            if getattr(self, "delta_x", None) is None:
                raise AttributeError("'CosmoBox' object has no attribute 'delta_k'")
            self._delta_k = self.engine.fft_r2c(self.delta_x)
        return self._delta_k

    @delta_k.setter
    def delta_k(self, value):
        self._delta_k = None if value is None else self._as_spectrum(value)

    def to_k(self, field):
        """fftn(field) of a real field as a device half spectrum (what callers of the reference write as
        ``np.fft.fftn(field)``), formed on first use: ``apply_transfer_fn`` + ``binned_power_spectrum`` of
        it run as one forward transform with the filter and the binning inside its last pass."""
        real = self._as_real(field)
        return LazySpectrum(self.engine, HALF, lambda: self.engine.fft_r2c(real), source_real=real)

    def to_real(self, field_k):
        """Real part of ifftn(field_k) as a device field (what callers of the reference
        write as ``np.fft.ifftn(box.velocity_k[2]).real``)."""
        if isinstance(field_k, LazySpectrum) and field_k.recipe is not None and not field_k.materialised:
            # velocity of a device-RNG realisation: regenerate delta_k inside the first inverse pass
            amp_key, seed, realisation, comp, fac = field_k.recipe
            self._set_amplitude(*amp_key)
            if comp == 2 and self.engine.fuses_redshift_space:
                # v_z: the last passes are deferred -- redshift_space_density of it can then finish them inside its own
                # kernel (RedshiftSpaceField); reading the field runs them as before
                wbox = weakref.ref(self)

                def again():
                    box = wbox()
                    if box is None:
                        raise RuntimeError("the CosmoBox that drew this field is gone; it cannot be drawn again")
                    box._set_amplitude(*amp_key)
                    return box.engine.realise_velocity_fused(seed, realisation, comp, fac)
                return PendingDensity(self.engine, self.engine.realise_velocity_begin(seed, realisation, comp, fac),
                                      regenerate=again)
            return self.engine.realise_velocity_fused(seed, realisation, comp, fac)
        f = self._as_spectrum(field_k)
        if f.kind == HALF:
            return self.engine.fft_c2r(f)
        full = self.engine.fft_c2c(f, +1, 1.0 / self.N ** 3)
        return self.engine.upload(full.host().real, REAL)

    # --------------------------------------------------------- Gaussian realisation
    def _power(self, k, scale_factor, linear):
        fn = _ccl.linear_matter_power if linear else _ccl.nonlin_matter_power
        return fn(self.cosmo, k=k, a=scale_factor)

    def _set_amplitude(self, scale_factor, linear):
        """sqrt(nan_to_num(P(k)) * boxfactor), box.py:161-171, on unique |k| shells for a
        cubic box, per stored mode otherwise."""
        key = (float(scale_factor), bool(linear))
        if key == self._amp_key:
            return
        N = self.N
        with np.errstate(all="ignore"):
            if self._cubic:
                n2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
                k = 2. * np.pi * np.sqrt(n2) / self.Lx
                pk = np.nan_to_num(np.asarray(self._power(k, scale_factor, linear), dtype=np.float64))
                amp = np.sqrt(pk * self.boxfactor)
                self.engine.set_amplitude_shells(amp)
                self._sigma2 = hostgeom.field_variance_cubic(N, amp)       # variance of the fields drawn from it
            else:
                # |k| depends on the mode numbers only through |m_x|, |m_y|, |m_z|: evaluate P(k) on the
                # (N/2+1)^3 magnitudes (an eighth of the stored modes), in the reference's operation order
                M = N // 2 + 1
                a = self._axis2
                s = (a[:M, None, None] + a[N:N + M][None, :, None]) + a[2 * N:2 * N + M][None, None, :]
                k = 2. * np.pi * np.sqrt(s)
                pk = np.nan_to_num(np.asarray(self._power(k.flatten(), scale_factor, linear), dtype=np.float64))
                amp = np.sqrt(pk.reshape(k.shape) * self.boxfactor)
                self.engine.set_amplitude_sym(amp)
                self._sigma2 = hostgeom.field_variance_sym(N, amp)
        self._amp_key = key

    def realise_density(self, linear=False, redshift=None, inplace=True):
        """Gaussian random field with the matter power spectrum (box.py:130-194).

        rng='numpy': ``re`` then ``im`` are drawn from the legacy global numpy stream
        exactly as the reference does, so ``np.random.seed(s)`` gives the same field.
        Conscious fix: with ``inplace=False`` the reference transforms a *stale*
        ``self.delta_k`` (box.py:187); here the new field is returned.
        """
        if redshift is None:
            redshift = self.redshift
        scale_factor = 1. / (1. + redshift)
        self._set_amplitude(scale_factor, linear)
        eng = self.engine
        N = self.N
        if self.rng == "numpy":
            re = eng.upload(np.random.normal(0.0, 1.0, (N, N, N)), REAL)
            im = eng.upload(np.random.normal(0.0, 1.0, (N, N, N)), REAL)
            half = eng.colour_noise(re, im)
            del re, im
            delta_x = eng.fft_c2r(half, destroy=True)
            delta_x.sigma2 = self._sigma2
        elif self._plain:
            # no fused generator pass on such a grid: the coloured half spectrum (same counters, same numbers), then c2r
            delta_x = eng.fft_c2r(eng.colour_device(self.seed, self._realisation), destroy=True)
            delta_x.sigma2 = self._sigma2
            self.last_realisation = self._realisation
            self._realisation += 1
        else:
            # generator fused into the first inverse FFT pass (no coloured spectrum round trip); the
            # last pass is deferred so that a following P(k) can fuse it with its own first pass
            amp_key, seed, real = self._amp_key, self.seed, self._realisation
            wbox = weakref.ref(self)      # (no reference cycle box -> delta_x -> closure -> box: a dropped field must
                                          # give its buffer back at once, not at the next garbage collection)

            def again():
                box = wbox()
                if box is None:
                    raise RuntimeError("the CosmoBox that drew this field is gone; it cannot be drawn again")
                box._set_amplitude(*amp_key)
                return box.engine.realise_fused(seed, real)
            delta_x = PendingDensity(eng, eng.realise_begin(seed, real), generator=(amp_key, seed, real),
                                     regenerate=again, sigma2=self._sigma2)
            self.last_realisation = self._realisation
            self._realisation += 1
        if inplace:
            if redshift != self.redshift:
                print("Warning: Storing density field into self.delta_x with a "
                      "different redshift than self.redshift.")
            self.delta_x = delta_x
            self._delta_k = None          # = fftn(delta_x), materialised on demand
        return delta_x

    def realisation_spectra(self, count, nbins=20, kbins=None, lognormal=False, linear=False, redshift=None, stride=1):
        """Additive (a Monte-Carlo loop in one call): P(k) of the next `count` realisations of this box's device generator
        -- indices r, r + stride, ... from the box's counter -- as ``(kc, pk[count, nbins-1], stddev[count, nbins-1])``.
        The same numbers, realisation by realisation, as

            dx = box.realise_density(); box.binned_power_spectrum(delta_x=box.lognormal(dx) if lognormal else dx, nbins=nbins)

        (box.py:130-194, :441-460, :696-768), but queued by the library itself (fb_montecarlo_power), which is what a
        small box's step is bound by; the fields are not kept (``box.delta_x`` is left as it was).  Cubic boxes on a
        power-of-two grid with rng='device'; anything else runs the loop above."""
        count, stride = int(count), int(stride)
        if count < 0 or stride < 1:
            raise ValueError("count >= 0 and stride >= 1")
        if redshift is None:
            redshift = self.redshift
        bins, kc, thr, amb = self._bin_setup(nbins, kbins)
        first = self._realisation
        fast = self.rng == "device" and not self._plain and thr is not None and (not lognormal or bins[0] > 0.)

        def one_by_one(indices):
            rows = []
            for r in indices:
                self._realisation = r
                dx = self.realise_density(linear=linear, redshift=redshift, inplace=False)
                rows.append(self.binned_power_spectrum(delta_x=self.lognormal(dx) if lognormal else dx, nbins=nbins, kbins=kbins,
                                                       keep_field=False))
            return rows
        if not fast:
            if self.rng != "device":
                raise ValueError("realisation_spectra needs rng='device' (realisations addressed by index)")
            rows = one_by_one([first + i * stride for i in range(count)])
            self._realisation = first + count * stride
            return kc.copy(), np.array([r[1] for r in rows]).reshape(count, -1), np.array([r[2] for r in rows]).reshape(count, -1)
        self._set_amplitude(1. / (1. + redshift), linear)
        eng = self.engine
        eng.set_bins(bins, thr, amb)
        nb = bins.size
        nvox = float(self.N) ** 3
        shift = hostgeom.lognormal_shift(self._sigma2, nvox) if lognormal else 0.0
        R = eng.montecarlo_power(self.seed, first, count, stride=stride, pre_exp=lognormal, exp_shift=shift)
        self._realisation = first + count * stride
        self.last_realisation = self._realisation - stride if count else getattr(self, "last_realisation", None)
        s1, s2, esum = R[:, 0:2 * nb:2], R[:, 1:2 * nb:2], R[:, 2 * nb]
        cnt = eng.bin_counts()
        good = np.ones(count, dtype=bool)
        with np.errstate(all="ignore"):
            if lognormal:
                good = hostgeom.lognormal_sums_in_range_many(cnt, s1, s2, esum)
                mean = esum / nvox
                s1, s2 = hostgeom.lognormal_rescale(s1, s2, mean)
            vals, std = hostgeom.finish_bins_many(cnt, s1, s2, self.boxfactor, _eps_of(eng))
        for i in np.nonzero(~good)[0]:
            # a realisation whose extremes fall outside what the variance-based shift allows for: once more on its own, where
            # the step is repeated with the shift from its maximum (binned_power_spectrum)
            keep = self._realisation
            row = one_by_one([first + int(i) * stride])[0]
            self._realisation = keep
            vals[i], std[i] = row[1], row[2]
        return kc.copy(), vals, std

    # ----------------------------------------------------------- velocity / potential
    def _field_k(self, delta_x, delta_k):
        if delta_x is not None and delta_k is not None:
            raise ValueError("delta_x and delta_k specified; can only specify one")
        if delta_x is not None:
            return self.engine.fft_r2c(self._as_real(delta_x))
        if delta_k is None:
            return self.delta_k
        return self._as_spectrum(delta_k)

    def realise_velocity(self, delta_x=None, delta_k=None, redshift=None, inplace=True):
        """v(k) = i [f H a] delta_k k_vec / k^2 per component (box.py:197-290)."""
        if redshift is None:
            redshift = self.redshift
        scale_factor = 1. / (1. + redshift)
        if delta_x is not None and delta_k is not None:
            raise ValueError("delta_x and delta_k specified; can only specify one")
        if self.N % 2 != 0:
            raise UnboundLocalError("local variable 'mx' referenced before assignment")
        fac = 100. * self.cosmo['h'] * _ccl.h_over_h0(self.cosmo, a=scale_factor) \
            * _ccl.growth_rate(self.cosmo, a=scale_factor) * scale_factor
        src = getattr(self, "delta_x", None)
        if delta_x is None and delta_k is None and self._delta_k is None \
                and isinstance(src, PendingDensity) and src.generator is not None:
            # the stored realisation came from the counter-based generator: delta_k = fftn(delta_x) is only
            # formed if a component is read in k space; to_real() regenerates it inside its first FFT pass
            box, cache = self, {}

            def dk_of():
                if "dk" not in cache:
                    cache["dk"] = box._delta_k if box.delta_x is src and box._delta_k is not None \
                        else box.engine.fft_r2c(src)
                return cache["dk"]
            velocity_k = tuple(LazySpectrum(self.engine, HALF, lambda c=c: self.engine.velocity_k(dk_of(), c, fac),
                                            recipe=src.generator + (c, fac)) for c in range(3))
        else:
            dk = self._field_k(delta_x, delta_k)
            velocity_k = tuple(LazySpectrum(self.engine, dk.kind, lambda c=c: self.engine.velocity_k(dk, c, fac))
                               for c in range(3))    # each component is computed when first used
        if inplace:
            self.velocity_k = velocity_k
        return velocity_k

    def realise_potential(self, delta_x=None, delta_k=None, redshift=None, inplace=True):
        """delta_k / k^2 with the monopole zeroed; like the reference the physical
        prefactor is not applied (box.py:344-348)."""
        dk = self._field_k(delta_x, delta_k)
        phi_k = self.engine.potential_k(dk)
        if inplace:
            self.phi_k = phi_k
        return phi_k

    # ------------------------------------------------------------------- filters
    def _filter_table(self, transfer_fn, layout_kind):
        """Evaluate an arbitrary callable on the host grid (as box.py:374-378 does)."""
        N = self.N
        m = self._modes
        ones = np.ones((N, N, N))
        k_perp = 2. * np.pi * np.sqrt(((m / self.Lx) ** 2.)[:, None, None] + ((m / self.Ly) ** 2.)[None, :, None]) * ones
        k_par = (2. * np.pi * m / self.Lz)[None, None, :] * ones
        with np.errstate(all="ignore"):
            t = np.asarray(transfer_fn(k_perp, k_par))
        if np.iscomplexobj(t):
            raise TypeError("complex-valued transfer functions are not supported on the device")
        t = np.broadcast_to(t, (N, N, N)).astype(self.engine.rdtype)
        if layout_kind == HALF:
            padded = np.zeros((N, self.engine.rows, self.engine.pitch), dtype=self.engine.rdtype)
            padded[:, :N, :N // 2 + 1] = t[:, :, :N // 2 + 1]
            t = padded
        return self.engine.upload_raw(t)

    def apply_transfer_fn(self, field_k, transfer_fn):
        """ifftn(nan_to_num(field_k * T(k_perp, k_par))) (box.py:356-381); the result is
        complex like the reference's.  A Hermitian (device half-spectrum) field with a
        ``DeviceFilter`` that is even in k_par takes the real-field fast path."""
        eng = self.engine
        f = self._as_spectrum(field_k)
        if isinstance(transfer_fn, DeviceFilter):
            if f.kind == HALF and transfer_fn.even_in_kpar:
                return FilteredField(eng, f, transfer_fn)      # lazy: see the class
            if f.kind == HALF:
                f = eng.expand_half(f)
            dk = eng.apply_filter(f, transfer_fn.kind, transfer_fn.params)
        else:
            if f.kind == HALF:
                f = eng.expand_half(f)     # an arbitrary callable need not be even in k_par
            table = self._filter_table(transfer_fn, FULL)
            dk = eng.apply_filter(f, FB_FILT_TABLE, table=table)
        if dk.kind == HALF:
            return eng.fft_c2r(dk, destroy=True, as_complex=True)
        return eng.fft_c2c(dk, +1, 1.0 / self.N ** 3, inplace=True)

    apply_filter = apply_transfer_fn

    def window(self, k, R):
        """Top-hat window squared (box.py:595-613)."""
        return self.window1(k, R) ** 2.

    def window1(self, k, R):
        """Top-hat window (box.py:615-633)."""
        x = k * R
        return (3. / x ** 3.) * (np.sin(x) - x * np.cos(x))

    def smooth_field(self, field_k, R):
        """Top-hat smoothing with radius R Mpc/h (box.py:635-655)."""
        eng = self.engine
        f = self._as_spectrum(field_k)
        dk = eng.apply_filter(f, FB_FILT_TOPHAT, (R / self.cosmo['h'], 0, 0, 0))
        if dk.kind == HALF:
            return eng.fft_c2r(dk, destroy=True, as_complex=True)
        return eng.fft_c2c(dk, +1, 1.0 / self.N ** 3, inplace=True)

    # ---------------------------------------------------------------- redshift space
    def redshift_space_density(self, delta_x=None, velocity_z=None, sigma_nl=0., method='linear'):
        """Line-of-sight remap to redshift space (box.py:384-438).  ``method`` is what the reference hands to scipy's
        ``griddata`` (box.py:433-437), all three of its one-dimensional rules on the device: 'linear' (default), 'nearest', and
        'cubic' -- the not-a-knot cubic spline through every line of sight's sorted shifted samples (what
        ``griddata(method='cubic')`` = ``interp1d(kind='cubic')`` is in one dimension), the fill value outside them."""
        if method not in self.engine.RSD_METHODS:
            raise ValueError("Unknown interpolation method %r for 1 dimensional data" % (method,))      # scipy's own refusal
        Hz = 100. * self.cosmo['h'] * _ccl.h_over_h0(self.cosmo, self.scale_factor)
        d = self._as_real(delta_x)
        v = self._as_real(velocity_z)
        noise = None
        if sigma_nl > 0. and self.rng == "numpy":
            # the reference draws N normals per line of sight in (i, j) order (box.py:416-418)
            noise = self.engine.upload(np.random.normal(0., 1., (self.N, self.N, self.N)), REAL)
        seed = self.seed + 0x9E3779B97F4A7C15 * (self._realisation + 1)
        if noise is None and method != "cubic" and self.engine.fuses_redshift_space:
            lazy = RedshiftSpaceField(self.engine, d, v, (Hz, sigma_nl, seed, method))
            if lazy.fusable():
                return lazy
        return self.engine.redshift_space(d, v, Hz, sigma_nl, noise, seed, method)

    # ------------------------------------------------------------------- COLA
    COLA_MAX_N = 1024

    def realise_density_cola(self, redshift=None, redshift_init=15., keep_velocities=True, seed=None, inplace=True,
                             n_steps=None, delta_lin=None, return_particles=False):
        """Density (and velocities) of a COLA particle-mesh run on the device (box.py:463-589, which calls pycola3): N^3
        particles on the box's grid, 2LPT initial positions at redshift_init, ``n_steps`` kick-drift-kick steps uniform in a
        (None: ``int(1 + redshift_init)``, as the reference; 0: pure 2LPT at ``redshift``), CIC painting.  Definition and
        deviations in DESIGN.md section 4.

        Initial conditions: ``delta_lin`` (host array or real DeviceArray, the z = 0 linear density) or the box's own linear
        field -- what ``realise_density(linear=True, redshift=0., inplace=False)`` would give now.  ``seed`` int: rng='numpy'
        draws re, then im from ``np.random.RandomState(seed)``; rng='device' uses Philox (seed, realisation 0); neither
        touches the global stream or the box's realisation counter.

        Returns delta_x, or (delta_x, vel_x, vel_y, vel_z) with ``keep_velocities`` -- real DeviceArrays; velocities are
        a dx/dt in km/s, painted with CIC and divided by the painted count (0 in empty cells).  ``return_particles`` appends a
        ``ColaParticles`` (fp64 positions in Mpc and velocities in km/s on the device)."""
        from . import cola
        from .halos import ColaParticles
        assert self.Lx == self.Ly == self.Lz, \
            "realise_density_cola() requires a cubic box with Lx=Ly=Lz"
        if redshift is None:
            redshift = self.redshift
        assert redshift_init > redshift, "Must have redshift_init > redshift"
        n_steps = int(1 + redshift_init) if n_steps is None else int(n_steps)
        if n_steps < 0:
            raise ValueError("n_steps must be >= 0")
        if self.N > self.COLA_MAX_N:
            raise ValueError("realise_density_cola: a %d^3 run needs about %.0f GB of device memory; grids up to %d^3 are "
                             "supported" % (self.N, cola.device_bytes(self.N, self.engine.precision, keep_velocities,
                                                                      return_particles) / 1e9, self.COLA_MAX_N))
        eng, N = self.engine, self.N
        d0 = self._as_real(delta_lin) if delta_lin is not None else self._cola_linear_field(seed)
        growth = cola.Growth(self.cosmo, _ccl)
        st = eng.cola_run(d0, n_steps, cola.launch_table(growth, redshift, redshift_init, n_steps))
        del d0
        delta_x = st["delta"]
        out = [delta_x]
        if keep_velocities or return_particles:
            P1, P2, fac = cola.velocity_coefficients(growth, redshift, self.cosmo['h'])
            pvel = eng._alloc_bytes(24 * N ** 3) if return_particles else None
            if keep_velocities:
                vbuf = eng._alloc_bytes(8 * N ** 3)
                for c in range(3):
                    eng.cola_velocity(st, c, P1, P2, fac, vbuf.ptr)
                    out.append(eng.cola_grid_velocity(st, vbuf.ptr))
                del vbuf
            if return_particles:
                for c in range(3):
                    eng.cola_velocity(st, c, P1, P2, fac, pvel.ptr + 8 * c, 3)
                out.append(ColaParticles(eng, st["pos"], N ** 3, pvel))
        del st
        eng.sync()
        if inplace:
            self.delta_x = delta_x
            self._delta_k = None
        return out[0] if len(out) == 1 else tuple(out)

    def _cola_linear_field(self, seed):
        """The z = 0 linear density of realise_density_cola (see there)."""
        if seed is None:
            return self.realise_density(linear=True, redshift=0., inplace=False)
        eng, N = self.engine, self.N
        self._set_amplitude(1.0, True)
        if self.rng == "numpy":
            rs = np.random.RandomState(int(seed))
            re = eng.upload(rs.normal(0.0, 1.0, (N, N, N)), REAL)
            im = eng.upload(rs.normal(0.0, 1.0, (N, N, N)), REAL)
            return eng.fft_c2r(eng.colour_noise(re, im), destroy=True)
        return eng.fft_c2r(eng.colour_device(int(seed), 0), destroy=True)

    # ------------------------------------------------------------------- log-normal
    def lognormal(self, delta_x):
        """exp(delta)/<exp(delta)> - 1 (box.py:441-460).  Returned lazily: the field is
        computed when it is first read, and ``binned_power_spectrum(delta_x=...)`` of it
        fuses the exp() into the first FFT pass instead of materialising it."""
        return LognormalField(self.engine, self._as_real(delta_x))

    # ----------------------------------------------------------------- power spectrum
    def _shell_thresholds(self, bins):
        """Bin as a step function of the integer shell n^2 (cubic boxes).  A shell whose
        |k| is within rounding of an edge is left to the exact on-device expression."""
        N = self.N
        n2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
        k = 2. * np.pi * np.sqrt(n2) / self.Lx
        eps = 64 * np.finfo(np.float64).eps
        lo = np.digitize(k * (1. - eps), bins)
        hi = np.digitize(k * (1. + eps), bins)
        amb = np.nonzero(lo != hi)[0]
        if amb.size > 8:
            return None, ()
        thr = np.searchsorted(hi, np.arange(1, bins.size + 1), side="left")
        return thr.astype(np.int32), tuple(int(a) for a in amb)

    def _bin_setup(self, nbins, kbins):
        """Edges, centres of bins 1..nbins-1 (box.py:745-751) and the shell thresholds, remembered per
        bin set: a Monte-Carlo loop asks for the same bins every realisation."""
        key = ("n", int(nbins)) if kbins is None else ("k", np.asarray(kbins, dtype=np.float64).tobytes())
        hit = self._bin_cache.get(key)
        if hit is not None:
            return hit
        if kbins is not None:
            bins = np.array(kbins, dtype=np.float64)
        else:
            bins = np.logspace(np.log10(self.kmin), np.log10(self.kmax), nbins)   # box.py:749
        _bins = [0.0] + list(bins)
        cent = [0.5 * (_bins[j + 1] + _bins[j]) for j in range(bins.size)]
        kc = np.array(cent[1:])
        thr, amb = (None, ())
        if self._cubic and np.all(np.diff(bins) >= 0):
            thr, amb = self._shell_thresholds(bins)
        bins.setflags(write=False)
        if len(self._bin_cache) > 16:
            self._bin_cache.clear()
        self._bin_cache[key] = (bins, kc, thr, amb)
        return self._bin_cache[key]

    def binned_power_spectrum(self, delta_x=None, delta_k=None, nbins=20, kbins=None, wait=True, keep_field=True):
        """Shell-averaged power spectrum of the realisation (box.py:696-768): bin centres,
        mean of |delta_k|^2/boxfactor and std/sqrt(n) per bin; bin 0 is dropped and empty
        bins are NaN, as in the reference.  ``wait=False`` (additive) returns a
        ``PendingSpectrum`` at once; its ``result()`` gives the same triple later, so that
        many realisations can be queued without a host round trip each.
        ``keep_field=False`` (additive; device-generator realisations whose last pass is still pending): the fused
        z pass does not write delta_x -- a Monte-Carlo loop that only wants spectra saves an eighth of the step's
        traffic; reading the field afterwards draws the same realisation again (same seed, same index)."""
        if delta_x is not None and delta_k is not None:
            raise ValueError("delta_x and delta_k specified; can only specify one")
        bins, kc, thr, amb = self._bin_setup(nbins, kbins)
        kc = kc.copy()                    # callers own what they get back
        eng = self.engine
        eng.set_bins(bins, thr, amb)

        if isinstance(delta_x, FilteredField):
            # P(k) of apply_transfer_fn's result = shell sums of |field_k T|^2 (Hermitian field, even filter)
            root, src = delta_x._root(), delta_x.spectrum
            filt = (delta_x.filter.kind, delta_x.filter.params)
            if root._x_done is None and not root.materialised and thr is not None \
                    and isinstance(src, LazySpectrum) and src.source_real is not None and not src.materialised:
                # what apply_transfer_fn returns is the field (box.py:381): the pass that filters and bins an x line
                # also transforms it back, and reading the field later costs the y and z passes only
                rs = src.source_real
                if isinstance(rs, RedshiftSpaceField) and rs.fusable():
                    res, root._x_done = rs.consume(filt, field=True)       # the z passes of the whole chain in one kernel
                else:
                    res, root._x_done = eng.power_filtered(rs, filt, field=True)
                pending = PendingSpectrum(eng, res, bins.size, kc, self.boxfactor, None, None)
                return pending if not wait else pending.result()
            cnt, s1, s2 = eng.bin_power(src, filt=filt)
            out = (kc,) + _finish_bins(cnt, s1, s2, self.boxfactor, _eps_of(eng))
            return out if wait else _Ready(out)

        if delta_x is None and delta_k is None and thr is not None and self._delta_k is None \
                and getattr(self, "delta_x", None) is not None:
            # the stored realisation, whose fftn has not been asked for yet (box.py:736-739 would use
            # self.delta_k = fftn(delta_x)): same numbers through the fused path below, no spectrum stored
            delta_x = self.delta_x
        if delta_x is not None and thr is not None:
            # fused path (cubic boxes): r2c with the binning inside the last pass
            ln = isinstance(delta_x, LognormalField) and not delta_x.materialised and bins[0] > 0.
            src = delta_x.source if ln else self._as_real(delta_x)
            # log-normal: exp(d - shift) instead of exp(d) -- the estimate exp(d)/<exp(d)> - 1 is the same, and with the
            # right shift a single-precision plan's sums stay inside the float range (a non-linear P(k) sampled at
            # 2 Mpc gives sigma = 8, exp(d) reaches 1e19 and |delta_k|^4 would overflow; at 0.5 Mpc sigma = 21).  A field
            # this box drew carries the variance of its distribution: the shift comes from that without a look at the
            # data (hostgeom.lognormal_shift; a realisation whose extremes fall outside is repeated with the exact shift,
            # PendingSpectrum.result).  Any other field is asked for its maximum first.
            shift, redo = 0.0, None
            if ln:
                nvox = float(self.N) ** 3
                sigma2 = getattr(src, "sigma2", None)
                if sigma2 is not None:
                    shift = hostgeom.lognormal_shift(sigma2, nvox)
                elif eng.precision == "f64":
                    shift = 0.0       # double precision needs no shift until exp(d) itself leaves the range (where the reference's
                                      # float64 does too), and a look at the data would wait for the stream (wait=False pipelines)
                else:
                    shift = hostgeom.lognormal_shift_exact(eng.max_real(src), nvox)
                nb_, bin_args = bins.size, (bins, thr, amb)
                # (the repeat must not keep the field alive: a loop that queues hundreds of spectra drops each delta_x
                # at once, and its buffer goes back to the pool; a field that is gone is drawn again from its recipe)
                wsrc, regen = weakref.ref(src), getattr(src, "_regenerate", None)

                def redo():
                    field = wsrc()
                    if field is None:
                        if regen is None:
                            raise FloatingPointError("log-normal P(k): the exponentials left the plan's floating-point "
                                                     "range and the field is no longer there to repeat the step")
                        field = regen()
                    self.lognormal_repeats += 1
                    eng.set_bins(*bin_args)
                    exact = hostgeom.lognormal_shift_exact(eng.max_real(field), nvox)   # (materialises a pending field)
                    res2, _ = eng.power_fused(field, pre_exp=True, exp_shift=exact)
                    return eng.fetch_results(res2, nb_)
            if isinstance(src, RedshiftSpaceField) and src.fusable() and not ln:
                res, _ = src.consume()
            elif isinstance(src, PendingDensity) and not src.materialised and src._pending is not None:
                res, real = eng.power_pending(src._pending, pre_exp=ln, exp_shift=shift, keep_field=keep_field)     # z passes fused
                if real is not None:
                    src._adopt(real)
                else:
                    src._pending = None        # consumed; reading the field later regenerates it
            else:
                res, _ = eng.power_fused(src, pre_exp=ln, exp_shift=shift)
            pending = PendingSpectrum(eng, res, bins.size, kc, self.boxfactor, self.N ** 3 if ln else None, None, redo)
            return pending if not wait else pending.result()

        if delta_x is not None:
            spec = eng.fft_r2c(self._as_real(delta_x))
        elif delta_k is None:
            spec = self.delta_k
        else:
            spec = self._as_spectrum(delta_k)
        cnt, s1, s2 = eng.bin_power(spec)
        out = (kc,) + _finish_bins(cnt, s1, s2, self.boxfactor, _eps_of(eng))
        return out if wait else _Ready(out)

    # ------------------------------------------------------------ correlation function
    def correlation_function(self, delta_x=None, second=None, dr=None, rmin=0., rmax=None, rbins=None, poles=None):
        """Additive: the two-point correlation function of a real field (or the cross-correlation with ``second``), what the
        reference's examples take from nbodykit as ``FFTCorr(first=mesh, mode='1d', los=[0,0,1], dr=, rmin=, rmax=)``
        (examples/example_corr_fn.py:38-47; step (6) of the end-to-end notebooks).  Returns ``(r, xi, npairs)``:

            D_a = fftn(d_a - mean(d_a)),  xi(s) = ifftn(conj(D_1) D_2) / N^3   (periodic);
            s_a = m_a L_a / N (m_a the signed FFT index), mu = s_z / |s| (line of sight z),
            bin b = [e_b, e_b+1); npairs = cells per bin, r = mean |s| per bin,
            xi_l = (2l + 1) sum xi(s) L_l(mu) / npairs.

        ``delta_x`` (default ``self.delta_x``) and ``second`` take whatever ``binned_power_spectrum(delta_x=...)`` takes.
        Edges: ``rbins``, or np.arange(rmin, rmax + dr/2, dr) with dr = min(L)/N, rmax = min(L)/2 by default (N/2 bins); at
        most 1024 bins, so the defaults fit every grid up to 2048^3 (ValueError beyond).  ``poles``:
        None -> xi is the monopole, shape (nbins,); a list out of (0, 2, 4) -> shape (len(poles), nbins).  Empty bins are
        NaN in r and xi.  The box's state (delta_x, stored spectrum, realisation counter, P(k) bins) is left as it was."""
        N = self.N
        L = (self.Lx, self.Ly, self.Lz)
        edges = hostgeom.separation_edges(L, N, dr=dr, rmin=rmin, rmax=rmax, rbins=rbins)
        ps = hostgeom.check_poles(poles)
        d1, d2 = self._two_fields(delta_x, second)
        raw = self.engine.correlation(d1, d2, edges, max(ps))
        r, xi, npairs = hostgeom.finish_correlation(raw, edges.size - 1, ps)
        return r, (xi[0].copy() if poles is None else xi), npairs

    def _two_fields(self, delta_x, second):
        """The real device fields of a two-point estimate: ``delta_x`` (default self.delta_x) and ``second`` (or None).
        Shapes and owners are checked (ValueError) before anything is uploaded or evaluated."""
        N = self.N
        for name, f in (("delta_x", delta_x), ("second", second)):
            if f is None:
                continue
            if isinstance(f, DeviceArray):
                if f.engine is not self.engine or f.kind != REAL:
                    raise ValueError("%s: a real field of this box" % name)
            elif np.shape(f) != (N, N, N):
                raise ValueError("%s: expected an array of shape %s, got %s" % (name, (N, N, N), np.shape(f)))
        if delta_x is None:
            delta_x = getattr(self, "delta_x", None)
            if delta_x is None:
                raise ValueError("no delta_x: realise_density() first, or pass delta_x")
        d1 = self._as_real(delta_x)
        d2 = self._as_real(second) if second is not None else None
        return d1, d2

    # ------------------------------------------------------------ power spectrum in (k, mu) bins
    def power_spectrum(self, delta_x=None, second=None, mode='1d', dk=None, kmin=0., kmax=None, kbins=None, Nmu=5,
                       poles=None):
        """Additive: the power spectrum of a real field (or the cross spectrum with ``second``) in |k| or (|k|, mu) bins, with
        multipoles -- what the reference's examples take from nbodykit as ``FFTPower(first=, second=, mode='1d' | '2d',
        los=[0,0,1], Nmu=, dk=, kmin=, kmax=, poles=)`` (examples/example_box.py:48-52, examples/example_halos.py:46-52):

            D_a = rfftn(d_a) (unnormalised),  P(k) = (Lx Ly Lz / N^6) Re(conj(D_1) D_2)   (fp64);
            k_a = m_a (2 pi / L_a) (m_a the signed FFT index), mu = |k_z| / |k| (line of sight z);
            every mode of the full grid but k = 0; k bin [e_b, e_b+1), mu bins np.linspace(0, 1, Nmu + 1) (mu = 1 in the last);
            per cell: modes, k = mean |k|, mu = mean mu, power = mean P;
            P_l(k_b) = (2l + 1) sum P(k) L_l(mu) / modes over the 1-d bin, l in (0, 2, 4).

        ``mode='1d'``: returns ``(k, power, modes)`` of shape (nk,), or with ``poles`` (a subset of (0, 2, 4)) ``power`` of
        shape (len(poles), nk).  ``mode='2d'``: returns ``(k, mu, power, modes)``, each (nk, Nmu); ``poles`` is refused.
        Edges: ``kbins``, or np.arange(kmin, kmax + dk/2, dk) with dk = 2 pi / min(L), kmax = pi N / max(L) by default (N/2
        bins on a cube); at most 1024 bins, 1 <= Nmu <= 128 and nk * Nmu <= 5120 (nk * 3 <= 5120 with poles 2 or 4).  Empty
        cells are NaN in k, mu and power.  ``delta_x`` (default ``self.delta_x``) and ``second`` take whatever
        ``correlation_function`` takes.  The box's state (delta_x, stored spectrum, realisation counter, P(k) bins) is left
        as it was.  Bad arguments raise ValueError before any device work."""
        if mode not in ('1d', '2d'):
            raise ValueError("mode must be '1d' or '2d', got %r" % (mode,))
        edges = hostgeom.power_edges((self.Lx, self.Ly, self.Lz), self.N, dk=dk, kmin=kmin, kmax=kmax, kbins=kbins)
        hostgeom.mu_edges(Nmu)
        nk = edges.size - 1
        if mode == '2d':
            if poles is not None:
                raise ValueError("poles are a mode='1d' output")
            nmu, ps = int(Nmu), None
        else:
            nmu, ps = 1, (None if poles is None else hostgeom.check_poles(poles))
        lmax = 0 if ps is None else max(ps)
        hostgeom.check_power_layout(nk, nmu, lmax)
        d1, d2 = self._two_fields(delta_x, second)
        raw = self.engine.power_kmu(d1, d2, edges, nmu, lmax)
        k, mu, power, modes = hostgeom.finish_power(raw, nk, nmu, ps)
        if mode == '2d':
            return k, mu, power, modes
        return k[:, 0].copy(), (power[:, 0].copy() if ps is None else power), modes[:, 0].copy()

    # ------------------------------------------------------------ cylindrical power, multi-frequency angular power
    def cylindrical_power_spectrum(self, delta_x=None, second=None, kperp_bins=None, kpar_bins=None, dk_perp=None,
                                   kperp_min=0., kperp_max=None):
        """Additive: the cylindrical power spectrum P(k_perp, k_par) of a real field (or the cross spectrum with ``second``),
        line of sight z -- the plane in which the foreground wedge, a beam's cut-off and the damage of a cleaning step are read
        off.  With the conventions of ``power_spectrum``:

            D_a = rfftn(d_a) (unnormalised),  P(k) = (Lx Ly Lz / N^6) Re(conj(D_1) D_2)   (fp64);
            k_a = m_a (2 pi / L_a) (m_a the signed FFT index), k_perp = sqrt(k_x k_x + k_y k_y), k_par = |k_z|;
            every mode of the full grid but k = 0; bins [e_b, e_b+1) on both axes (np.digitize - 1), modes outside dropped;
            per cell: modes, kperp = mean k_perp, kpar = mean k_par, power = mean P.

        Returns ``(kperp, kpar, power, modes)``, each (nperp, npar), float64, writeable.  Edges: ``kperp_bins``, or
        np.arange(kperp_min, kperp_max + dk_perp/2, dk_perp) with dk_perp = 2 pi / min(Lx, Ly), kperp_max = pi N / max(Lx, Ly)
        by default; ``kpar_bins``, or one bin around every |m_z|: (np.arange(N/2 + 2) - 0.5) 2 pi / Lz (N/2 + 1 bins).  The last
        edge of either may be inf.  1 <= nperp <= 1024, 1 <= npar <= 1025; every grid.  Empty cells are NaN in kperp, kpar and
        power.  Sums are fp64 in a fixed order: two calls agree bit for bit.  ``delta_x`` (default ``self.delta_x``) and
        ``second`` take whatever ``power_spectrum`` takes.  The box's state (delta_x, stored spectrum, realisation counter,
        P(k) bins) is left as it was.  Bad arguments raise ValueError before any device work."""
        perp, par = hostgeom.cyl_edges((self.Lx, self.Ly, self.Lz), self.N, kperp_bins=kperp_bins, kpar_bins=kpar_bins,
                                       dk_perp=dk_perp, kperp_min=kperp_min, kperp_max=kperp_max)
        d1, d2 = self._two_fields(delta_x, second)
        raw = self.engine.power_cyl(d1, d2, perp, par)
        return hostgeom.finish_cyl(raw, perp.size - 1, par.size - 1)

    def angular_power_spectrum(self, delta_x=None, second=None, kperp_bins=None, dk_perp=None, kperp_min=None,
                               kperp_max=None, collapse=False, angular=False, redshift=None):
        """Additive: the multi-frequency angular power spectrum of a cube whose last axis is frequency (the flat-sky
        C_l(nu, nu') of Datta et al. 2007 and Mondal et al. 2018), or the cross spectrum with ``second``: the covariance of
        the channels per angular scale, which shows whether spectrally smooth components were removed.

            a_a(m_perp, nu) = np.fft.fftn(d_a, axes=(0, 1)) (unnormalised), every m_perp of the N x N plane but m_perp = 0;
            C_b(nu, nu') = (Lx Ly / N^4) (1 / modes_b) sum_{m_perp in b} Re(a_1(m_perp, nu) conj(a_2(m_perp, nu')));
            k_perp and its bins as in ``cylindrical_power_spectrum``.

        Returns ``(kperp, cl, modes)``: kperp (nb,) the mean k_perp of each bin, cl (nb, N, N) float64 in Mpc^2 x field^2,
        modes (nb,) int64.  The first channel index belongs to ``delta_x``, the second to ``second``; the auto result is
        symmetric bit for bit.  Empty bins are NaN in kperp and cl.  Edges: ``kperp_bins``, or np.arange(kperp_min,
        kperp_max + dk_perp/2, dk_perp) with dk_perp = 2 pi / min(Lx, Ly), kperp_min = dk_perp / 2 for the default dk_perp
        (half the fundamental) and kperp_max = pi N / max(Lx, Ly); 1 <= nb <= 256, N <= 1024.  ``collapse=True``: cl is (nb, N),
        the mean of C_b(nu, nu + D) over the N - D pairs.  ``angular=True``: returns l = k_perp r and C / r^2 with
        r = comoving_angular_distance(cosmo, 1 / (1 + redshift)) (``redshift`` defaults to the box's), the distance
        ``pixel_array`` uses.  The work memory (a complex cube per field, the partial sums and the result) must fit in device
        memory: MemoryError before any kernel runs otherwise.  Operands are held in the box's precision, products and sums
        are fp64 on the matrix cores in a fixed order (two calls agree bit for bit).  The box's state is left as it was.  Bad
        arguments raise ValueError before any device work."""
        N = self.N
        edges = hostgeom.maps_edges((self.Lx, self.Ly, self.Lz), N, kperp_bins=kperp_bins, dk_perp=dk_perp,
                                    kperp_min=kperp_min, kperp_max=kperp_max)
        nb = edges.size - 1
        if angular:
            z = self.redshift if redshift is None else redshift
            if not np.isfinite(z) or z <= -1.:
                raise ValueError("redshift must be finite and > -1, got %r" % (redshift,))
        for name, f in (("delta_x", delta_x), ("second", second)):     # (the checks of _two_fields, ahead of the memory check)
            if isinstance(f, DeviceArray):
                if f.engine is not self.engine or f.kind != REAL:
                    raise ValueError("%s: a real field of this box" % name)
            elif f is not None and np.shape(f) != (N, N, N):
                raise ValueError("%s: expected an array of shape %s, got %s" % (name, (N, N, N), np.shape(f)))
        eng = self.engine
        need, have = eng.angular_power_bytes(nb, second is not None), eng.free_bytes()
        if need > have:
            raise MemoryError("angular_power_spectrum: %d bins of %d^2 channels and their work cubes take %.1f GiB, %.1f GiB "
                              "are free" % (nb, N, need / 2. ** 30, have / 2. ** 30))
        d1, d2 = self._two_fields(delta_x, second)
        raw, cl = eng.angular_power(d1, d2, edges)
        kperp, modes = hostgeom.finish_maps(raw, nb)
        if collapse:
            cl = hostgeom.collapse_maps(cl)
        if angular:
            r = _ccl.comoving_angular_distance(self.cosmo, 1. / (1. + z))
            return kperp * r, cl / r ** 2, modes
        return kperp, cl, modes

    # ------------------------------------------------------------ bispectrum in triangle bins
    def bispectrum(self, delta_x=None, kbins=None, dk=None, kmin=0., kmax=None, reduced=False):
        """Additive: the bispectrum of a real field in bins of three |k| shells, by the FFT estimator (Scoccimarro 2000;
        Sefusatti et al. 2016), with the conventions of ``power_spectrum``:

            D = fftn(d) (unnormalised; k = 0 never enters),  k_a = m_a (2 pi / L_a) (m_a the signed FFT index);
            shell S_b = every mode m != 0 of the full grid with |k| in [e_b, e_b+1);
            I_b(x) = sum over S_b of D(m) exp(+2 pi i m.x / N),  U_b the same with D = 1;
            for the shell triples b1 <= b2 <= b3 in itertools.combinations_with_replacement(range(nb), 3) order:
            ntri = sum_x U_b1 U_b2 U_b3 / N^3, the number of (m1, m2, m3) in S_b1 x S_b2 x S_b3 with m1 + m2 + m3 = 0
            modulo N on every axis;  B = (V^2 / N^12) sum_x I_b1 I_b2 I_b3 / ntri,  V = Lx Ly Lz;
            Q = B / (P1 P2 + P2 P3 + P3 P1) with P_b the mean of (V / N^6) |D|^2 over S_b.

        Returns ``(k, B, ntri)``, or ``(k, B, Q, ntri)`` with ``reduced=True``: ``k`` (T, 3) holds the mean |k| of each
        triple's shells, the others are (T,), T = nb (nb + 1) (nb + 2) / 6; float64, writeable.  Triples without a triangle
        are NaN in k, B and Q.  Triangles close modulo N, which is what the estimator computes: with the last edge at or below
        (2/3) pi N / max(L) no triangle closes through an alias.  Edges: ``kbins``; or np.arange(kmin, kmax + dk/2, dk) when
        ``dk`` is given; by default np.linspace(kmin, kmax, 17) with kmax = (2/3) pi N / max(L) (16 shells); 1 to 32 shells.
        The shell cubes are held in the box's precision, their products and sums are fp64 in a fixed order (two calls agree bit
        for bit); ntri is formed in fp64 whatever the precision, once per edge set.  The nb cubes must fit in device memory
        (8 GiB at 512^3 in single precision with 16 shells): MemoryError before any kernel runs otherwise.  ``delta_x``
        (default ``self.delta_x``) takes whatever ``power_spectrum`` takes.  The box's state (delta_x, stored spectrum,
        realisation counter, P(k) bins) is left as it was.  Bad arguments raise ValueError before any device work."""
        N = self.N
        L = (self.Lx, self.Ly, self.Lz)
        edges = hostgeom.bispectrum_edges(L, N, dk=dk, kmin=kmin, kmax=kmax, kbins=kbins)
        nb = edges.size - 1
        if N > 1024:
            raise ValueError("bispectrum: grids up to 1024^3")
        eng = self.engine
        need = eng.bispectrum_bytes(nb)
        if eng.precision != "f64" and edges.tobytes() not in self.__dict__.get("_bk_triangles", {}):
            need *= 2                                  # the triangle counts of a new edge set: the same cubes in fp64
        have = eng.free_bytes()
        if need > have:
            raise MemoryError("bispectrum: %d shell cubes and their work spectra take %.1f GiB, %.1f GiB are free"
                              % (nb, need / 2. ** 30, have / 2. ** 30))
        d1, _ = self._two_fields(delta_x, None)
        ntri = self._bispectrum_triangles(edges)
        raw = eng.bispectrum(d1, edges)
        k, B, Q, ntri = hostgeom.finish_bispectrum(raw, ntri, nb, L, N)
        return (k, B, Q, ntri) if reduced else (k, B, ntri)

    def _bispectrum_triangles(self, edges):
        """ntri of an edge set: from the unit spectrum on a double-precision plan of this grid (the box's own, or a twin of
        a single-precision box), rounded to integers and kept per edge set."""
        cache = self.__dict__.setdefault("_bk_triangles", {})
        key = edges.tobytes()
        if key not in cache:
            eng = self.engine
            if eng.precision != "f64":
                twin = eng.__dict__.get("_f64_twin")
                if twin is None:
                    twin = Engine(self.N, (self.Lx, self.Ly, self.Lz), self._axis2, self._ksc, self._kpar, self.z,
                                  precision="f64", device=eng.device, stream=(eng.stream.value if eng.stream else None))
                    eng.__dict__["_f64_twin"] = twin
                eng = twin
            if len(cache) >= 16:
                cache.pop(next(iter(cache)))
            cache[key] = hostgeom.bispectrum_ntri(eng.bispectrum(None, edges, unit=True), edges.size - 1, self.N)
            eng.release_idle_buffers()
        return cache[key]

    # ------------------------------------------------------------ painting a catalogue
    def paint_catalogue(self, positions, weights=None, window='cic', compensated=False):
        """Additive: mass assignment of a catalogue onto this box's grid, what the reference's examples take from nbodykit as
        ``ArrayCatalog({'Position': pos}).to_mesh(Nmesh=N, BoxSize=L, window=..., compensated=...)``
        (examples/example_halos.py).  ``positions``: a HaloCatalogue or a host (n, 3) array (comoving, periodic);
        ``weights``: optional length-n host array or float64 device tensor.  Returns a real DeviceArray holding
        sum(weight * W), node m at m L_a / N, u = x N / L_a:

            'ngp': node floor(u + 1/2);  'cic': floor(u), floor(u) + 1 with 1 - f, f;
            'tsc': floor(u + 1/2) + (-1, 0, 1) with (1/2 - d)^2 / 2, 3/4 - d^2, (1/2 + d)^2 / 2.

        ``compensated``: every Fourier mode divided by prod_a sinc(pi m_a / N)^p, p = 1, 2, 3.  The mesh is the same bit for
        bit from call to call (fixed-point accumulation).  Agreement with nbodykit itself is intended but unverified."""
        from . import halos
        return halos.paint(self, positions, weights=weights, window=window, compensated=compensated)

    # ------------------------------------------------------------ friends-of-friends halos
    def find_halos(self, particles, **kw):
        """Additive: the friends-of-friends halos of a particle set in this box -- the ``ColaParticles`` of
        ``realise_density_cola(return_particles=True)``, a HaloCatalogue or a host (n, 3) array -- as a ``FoFHalos``
        catalogue (centres of mass, counts, masses, mean velocities, per-particle labels), found on the device.  Keywords and
        definition: ``fastbox_amd.halos.find_halos_fof``; DESIGN.md section 4."""
        from . import halos
        return halos.find_halos_fof(self, particles, **kw)

    def pair_counts(self, first, second=None, edges=None, mode='1d', Nmu=10, pimax=None, poles=None):
        """Additive: pair counts of one catalogue (or of ``first`` against ``second``) in bins of r, (r, mu) or (r_p, pi),
        counted on the device, and xi = npairs / RR - 1 with the analytic RR of the periodic box -- what nbodykit's
        ``SimulationBox2PCF`` gives (the reference's examples/example_corr_fn.py leaves it commented out).  Catalogues: a
        ``FoFHalos``, ``ColaParticles`` or other HaloCatalogue of this box, or a host (n, 3) array.  Returns a ``PairCounts``.
        Keywords and definition: ``fastbox_amd.halos.pair_counts``; DESIGN.md section 4."""
        from . import halos
        return halos.pair_counts(self, first, second=second, edges=edges, mode=mode, Nmu=Nmu, pimax=pimax, poles=poles)

    def halo_profiles(self, centres, particles, edges, **kw):
        """Additive: radial profiles of all particles around given centres (a ``FoFHalos``, another HaloCatalogue or a host
        (nh, 3) array), counted on the device: a ``HaloProfiles`` of integer counts per bin, enclosed counts and densities.
        Keywords and definition: ``fastbox_amd.halos.halo_profiles``; DESIGN.md section 4."""
        from . import halos
        return halos.halo_profiles(self, centres, particles, edges, **kw)

    def spherical_overdensity(self, centres, particles, **kw):
        """Additive: spherical-overdensity radii R_Delta and masses M_Delta around given centres, with the exact members,
        centre of mass, mean velocity and velocity dispersion inside R_Delta, as an ``SOHalos`` catalogue (its positions are
        the centres).  Keywords and definition: ``fastbox_amd.halos.spherical_overdensity``; DESIGN.md section 4."""
        from . import halos
        return halos.spherical_overdensity(self, centres, particles, **kw)

    def triplet_multipoles(self, positions, edges, lmax=10, weights=None, probe=None, timings=None):
        """Additive: the raw three-point multipole moments M_l(b1, b2) of a weighted catalogue, its pair counts and, with
        ``probe``, the harmonic coefficients a_lm of chosen primaries, summed on the device.  Keywords and definition:
        ``fastbox_amd.halos.triplet_multipoles``; DESIGN.md section 4."""
        from . import halos
        return halos.triplet_multipoles(self, positions, edges, lmax=lmax, weights=weights, probe=probe, timings=timings)

    def three_point(self, data, edges, lmax=10, randoms=None, weights=None, seed=None):
        """Additive: the multipoles zeta_l(r1, r2), l <= ``lmax`` <= 10, of the configuration-space three-point correlation
        function of a catalogue in this periodic box -- what nbodykit's ``SimulationBox3PCF`` gives on the host -- by the
        algorithm of Slepian & Eisenstein (2015) on the device, O(n x neighbours).  ``data``: a ``ColaParticles``,
        ``FoFHalos``, ``SOHalos`` or other HaloCatalogue of this box, or a host (n, 3) array; ``weights``: n host values
        (default 1); ``edges``: up to 32 radial bins in Mpc, edges[0] > 0, the last edge below min(L) / 2.  ``randoms`` None:
        zeta = (2 l + 1) M_l / norm - [l = 0], the multipoles of the full three-point function; a number: that many uniform
        points per datum drawn on the device (``uniform_catalogue`` with ``seed``), or a catalogue / (n, 3) array: the randoms
        join the sweep with weight -W_d / n_r each and zeta = (2 l + 1) M_l / norm is the connected zeta_l of N = D - R
        (Szapudi & Szalay).  Data and randoms are joined on the device.  Returns a ``fastbox_amd.halos.ThreePoint``.
        Definition, normalisation and what is out of scope: DESIGN.md section 4.  Agreement with nbodykit is intended, not
        verified."""
        from . import halos
        return halos.three_point(self, data, edges, lmax=lmax, randoms=randoms, weights=weights, seed=seed)

    # ------------------------------------------------------------ density-field reconstruction and mesh readout
    def reconstruct(self, data, randoms=None, smoothing=10., bias=1., f=0., convention='sym', window='cic', delta=None,
                    seed=None, return_displacement=False):
        """Additive: density-field (BAO) reconstruction on the device -- what pyrecon's and nbodykit's FFT reconstruction give
        the host pipelines (Eisenstein et al. 2007; Padmanabhan et al. 2012; Burden et al. 2014); definition in DESIGN.md
        section 4.  delta = n / nbar - 1 of ``data`` painted with ``window`` (or the real mesh ``delta``, used as it is: a
        cleaned intensity map, say); Psi_a(k) = i k_a delta(k) exp(-k^2 R^2 / 2) / (b (k^2 + beta k_z^2)) with R = ``smoothing``
        (Mpc), b = ``bias``, beta = f / b, the line of sight along z; the data move to wrap(x - Psi(x) - f Psi_z(x) z^), the
        randoms likewise with ``convention='sym'`` (RecSym) and by -Psi alone with ``'iso'`` (RecIso); ``delta_rec`` =
        D / nbar_D - S / nbar_S of the two shifted sets painted with the same window.  ``data``: ColaParticles, FoFHalos,
        SOHalos or another HaloCatalogue of this box, or a host (n, 3) array (Mpc, periodic, wrapped on read).  ``randoms``:
        None: 4 n uniform points drawn on the device (Philox stream 10 with ``seed``, default the box's: the same points on
        every call); an integer: that many; 'grid': one on each mesh node, no shot noise; or a catalogue / (n, 3) array.
        Returns a ``fastbox_amd.recon.Reconstruction`` (delta_rec, the shifted data and randoms as HaloCatalogues, the
        displacement with ``return_displacement``).  ValueError / TypeError name the argument: positions that are not finite
        or have |x| >= 2^52 L, more than 2^31 - 2 particles, smoothing <= 0, bias <= 0, f < 0, an unknown convention or
        window, a complex ``delta``; MemoryError before any kernel runs if the work memory does not fit.  Agreement with
        pyrecon and nbodykit is intended, not verified."""
        from . import recon
        return recon.reconstruct(self, data, randoms=randoms, smoothing=smoothing, bias=bias, f=f, convention=convention,
                                 window=window, delta=delta, seed=seed, return_displacement=return_displacement)

    def readout(self, field, positions, window='cic'):
        """Additive: mesh -> particle interpolation, the adjoint of ``paint_catalogue``: the value of a real field of this
        box at each position through the window's nodes and weights ('ngp', 'cic', 'tsc'; fp64 weights on both precisions).
        ``field``: a real DeviceArray or host (N, N, N) array, or a list of up to three (a velocity, a displacement);
        ``positions``: a HaloCatalogue of this box or a host (n, 3) array, periodic.  Returns fp64 values on the device,
        shape (n,) or, for a list, (n, k); ``np.asarray`` copies them to the host."""
        from . import recon
        return recon.readout(self, field, positions, window=window)

    def uniform_catalogue(self, n, seed=None):
        """Additive: ``n`` points uniform in the box, drawn on the device (Philox stream 10; ``seed`` default the box's; every
        call without a seed of its own takes the box's next draw), as a HaloCatalogue.  Host model:
        ``fastbox_amd.rng.recon_uniforms(n, L, seed, realisation)`` with the catalogue's ``seed`` and ``realisation``."""
        from . import recon
        return recon.uniform_catalogue(self, n, seed=seed)

    # ------------------------------------------------------------ Minkowski functionals of excursion sets
    def minkowski_functionals(self, delta_x=None, **kw):
        """Additive: the Minkowski functionals of the excursion sets {delta_x >= t} -- volume fraction, surface, integrated
        mean curvature and Euler characteristic (genus) densities of the periodic box, or with ``per_channel=True`` the area,
        perimeter and Euler characteristic of every frequency channel -- from exact integer counts of the cell complex made
        in one pass on the device.  ``delta_x`` (default ``self.delta_x``): a real DeviceArray of this box or a host (N, N, N)
        real array; a complex field or a spectrum raises TypeError, another shape or box ValueError.  Keywords
        (``thresholds`` | ``nu``, ``per_channel``) and definition: ``fastbox_amd.minkowski.minkowski_functionals``; DESIGN.md
        section 4.  Returns a ``MinkowskiFunctionals``.  The box's state is left as it was."""
        from . import minkowski
        if delta_x is None:
            delta_x = getattr(self, "delta_x", None)
            if delta_x is None:
                raise ValueError("no delta_x: realise_density() first, or pass delta_x")
        return minkowski.minkowski_functionals(delta_x, box=self, **kw)

    # ------------------------------------------------------------ cosmic-web classification
    def tidal_tensor(self, delta_x=None, delta_k=None, smoothing=0.):
        """Additive: the tidal tensor of a density on the device, the inverse transforms of k_i k_j / k^2 exp(-k^2 R^2 / 2)
        delta(k) with R = ``smoothing`` (Mpc), as a ``fastbox_amd.web.TensorField`` (six real DeviceArrays xx, yy, zz, xy, xz,
        yz; ``trace()``).  ``delta_x`` (default ``self.delta_x``) or ``delta_k``, not both.  Definition and Nyquist rules:
        ``fastbox_amd.web.tidal_tensor``; DESIGN.md section 4.  The box's state is left as it was."""
        from . import web
        return web.tidal_tensor(self, delta_x=delta_x, delta_k=delta_k, smoothing=smoothing)

    def cosmic_web(self, delta_x=None, smoothing=0., threshold=0., kind='tidal', velocity=None, **kw):
        """Additive: the cosmic web of a field on the device -- every voxel a void, sheet, filament or knot by the number of
        eigenvalues above ``threshold`` of the tidal tensor of ``delta_x`` (``kind='tidal'``, the T-web; default
        ``self.delta_x``) or of the shear tensor of ``velocity``, three real cubes in km/s (``kind='shear'``, the V-web), both
        smoothed with a Gaussian of ``smoothing`` Mpc.  ``threshold``: a number, or up to 16 ascending ones for a scan.
        Keywords ``weight``, ``return_classes``, ``return_eigenvalues`` as ``fastbox_amd.web.classify``; ``H0`` (km/s/Mpc,
        default 100 h) with ``kind='shear'``.  Returns a
        ``fastbox_amd.web.CosmicWeb`` (counts, volume and mass fractions, the class cube and its masks).  ValueError /
        TypeError name the argument, before any device work; MemoryError if the work memory does not fit.  DESIGN.md
        section 4.  The box's state is left as it was."""
        from . import web
        return web.cosmic_web(self, delta_x=delta_x, smoothing=smoothing, threshold=threshold, kind=kind, velocity=velocity, **kw)

    def sigmaR(self, R):
        """RMS of the field smoothed with a top-hat of R Mpc/h, from the binned power
        spectrum (box.py:657-683; scipy's simps is spelled simpson since 1.14)."""
        k, pk, stddev = self.binned_power_spectrum()
        good = ~np.isnan(pk)
        pk, k = pk[good], k[good]
        y = k ** 2. * pk * self.window(k, R / self.cosmo['h'])
        I = _simpson(y, x=k)
        return np.sqrt(I / (2. * np.pi ** 2.))

    def sigma8(self):
        return self.sigmaR(8.0)

    def theoretical_power_spectrum(self):
        """box.py:770-782."""
        k = np.logspace(-3.5, 1., int(1e3))
        pk = _ccl.nonlin_matter_power(self.cosmo, k=k, a=self.scale_factor)
        return k, pk

    # ----------------------------------------------------------------- coordinates
    def freq_array(self, redshift=None):
        """Channel frequencies in MHz, decreasing along z (box.py:789-828)."""
        if redshift is None:
            redshift = self.redshift
        a = 1. / (1. + redshift)
        dx = self.Lz / self.N
        Hz = 100. * self.cosmo['h'] * _ccl.h_over_h0(self.cosmo, a)
        df = dx * self.line_freq * (a ** 2. * Hz) / (C / 1e3)
        freqs = a * self.line_freq + df * (np.arange(self.N) - 0.5 * (self.N - 1.))
        return freqs[::-1]

    def pixel_array(self, redshift=None):
        """Angular pixel coordinates in degrees (box.py:831-864)."""
        if redshift is None:
            redshift = self.redshift
        r = _ccl.comoving_angular_distance(self.cosmo, 1. / (1. + redshift))
        ang_x = (180. / np.pi) * ((self.x[1] - self.x[0]) / r)
        ang_y = (180. / np.pi) * ((self.y[1] - self.y[0]) / r)
        grid = np.arange(self.N) - 0.5 * (self.N - 1.)
        return ang_x * grid, ang_y * grid

    # ------------------------------------------------------------------ self tests
    def test_parseval(self):
        """sum(delta_x^2) N^3 against sum |delta_k|^2 (box.py:931-948), both reduced on
        the device in fp64."""
        s1 = self.engine.sum_real(self.delta_x, squared=True) * self.N ** 3.
        s2 = self.engine.sumsq_half(self.delta_k) if self.delta_k.kind == HALF \
            else float(np.sum(np.abs(self.delta_k.host()) ** 2))
        print("Parseval test:", s1 / s2, "(should be 1.0)")
        return s1, s2

    def test_sampling_error(self):
        """sigma8 of the realisation against theory (box.py:871-928)."""
        h = self.cosmo['h']
        s8_real = self.sigma8()
        _k = np.linspace(self.kmin, self.kmax, int(5e3))
        _pk = _ccl.nonlin_matter_power(self.cosmo, k=_k, a=self.scale_factor)
        _y = np.nan_to_num(_k ** 2. * _pk * self.window(_k, 8.0 / h))
        s8_th_win = np.sqrt(_simpson(_y, x=_k) / (2. * np.pi ** 2.))
        _k2 = np.logspace(-5, 2, int(5e4))
        _pk2 = _ccl.nonlin_matter_power(self.cosmo, k=_k2, a=self.scale_factor)
        _y2 = np.nan_to_num(_k2 ** 2. * _pk2 * self.window(_k2, 8.0 / h))
        s8_th_full = np.sqrt(_simpson(_y2, x=_k2) / (2. * np.pi ** 2.))
        s8_realspace = np.std(np.asarray(self.smooth_field(self.delta_k, 8.0)))
        s20_realspace = np.std(np.asarray(self.smooth_field(self.delta_k, 20.0)))
        s20_real = self.sigmaR(20.)
        print("")
        print("sigma8 (real.): \t", s8_real)
        print("sigma8 (th.win.):\t", s8_th_win)
        print("sigma8 (th.full):\t", s8_th_full)
        print("sigma8 (realsp.):\t", s8_realspace)
        print("ratio =", 1. / (s8_real / s8_realspace))
        print("")
        print("sigma20 (real.): \t", s20_real)
        print("sigma20 (realsp.):\t", s20_realspace)
        print("ratio =", 1. / (s20_real / s20_realspace))
        print("var(delta) =", np.sqrt(self.engine.sum_real(self.delta_x, True) / self.N ** 3
                                      - (self.engine.sum_real(self.delta_x) / self.N ** 3) ** 2))
