"""
Halo tracers on the device: the counterpart of the reference's fastbox/halos.py.

    from fastbox_amd.halos import HaloDistribution          # as fastbox.halos
    halos = HaloDistribution(box, mass_range=(1e12, 1e15), mass_bins=10)
    counts = halos.halo_count_field(box.delta_x, nbar=1e-3, bias=1.)      # real DeviceArray of integer counts
    cat = halos.realise_halo_catalogue(counts, scatter=True)               # HaloCatalogue, (Nh, 3) fp64 on the device
    mesh = box.paint_catalogue(cat, window='tsc', compensated=True)        # nbodykit's to_mesh

Random numbers follow the box, as in ``sky.py``: ``rng='numpy'`` draws the reference's legacy global stream on the host in
the reference's order (``np.random.seed(s)`` gives the reference's counts and catalogue); ``rng='device'`` draws Philox
streams 5 (counts) and 6 (catalogue offsets) on the device, reproduced by ``fastbox_amd.rng`` (``stream_poisson``,
``scatter_uniforms``).

Limits: an expected count above 2^24 raises ValueError, so that fp32 counts stay exact; a count drawn above 2^24 -- possible
from an expected count some 15-20 thousand below the limit, sigma being 4096 there -- is stored rounded to fp32, to an even
number, on a single-precision plan.  An
all-zero count field gives an empty (0, 3) catalogue, where the reference raises.
"""
import ctypes

import numpy as np

from . import _lib
from .device import DeviceArray, DeviceBuffer, REAL

LAM_MAX = float(2 ** 24)
WINDOWS = {"ngp": 0, "cic": 1, "tsc": 2}
_SCALAR, _ZPROFILE, _FIELD, _FIELD_F64 = 0, 1, 2, 3


class HaloCatalogue(DeviceBuffer):
    """Halo positions (comoving, Mpc) on the device: fp64 [Nh][3].  ``np.asarray(cat)`` is the (Nh, 3) array."""

    def __init__(self, engine, buf, n):
        self.n = int(n)
        DeviceBuffer.__init__(self, engine, buf, (self.n, 3), np.float64)

    def __repr__(self):
        return "HaloCatalogue(%d halos)" % self.n


class ColaParticles(HaloCatalogue):
    """The particles of CosmoBox.realise_density_cola: positions (Mpc, wrapped to [0, L)) as a HaloCatalogue -- so
    ``paint_catalogue`` takes them -- and ``velocities``, the peculiar velocities a dx/dt in km/s, fp64 (n, 3) on the device
    (``np.asarray(p.velocities)`` is the host copy)."""

    def __init__(self, engine, buf, n, vel_buf):
        HaloCatalogue.__init__(self, engine, buf, n)
        self.velocities = HaloCatalogue(engine, vel_buf, n)

    def __repr__(self):
        return "ColaParticles(%d particles)" % self.n


def _next_realisation(box):
    r = getattr(box, "_halo_draws", 0)
    box._halo_draws = r + 1
    return r


class HaloDistribution(object):

    def __init__(self, box, mass_range, mass_bins):
        """Halos on top of a realisation of a density field in ``box`` (a CosmoBox); mass_range (Msun) and mass_bins are kept
        as the reference keeps them."""
        self.box = box
        self.Mmin, self.Mmax = mass_range
        self.mass_bins = mass_bins
        self.last_realisation = None

    def construct_bins(self, z):
        raise NotImplementedError("construct_bins needs a halo mass function (pyccl), which this port does not have; the "
                                  "reference's version also uses an undefined `cosmo`")

    # ------------------------------------------------------------------ counts
    def _param(self, v, name, keep):
        """(pointer, kind, value) of nbar / bias: a scalar, a length-N profile along z, or an (N, N, N) host / device array."""
        box, eng = self.box, self.box.engine
        N = box.N
        if isinstance(v, DeviceArray):
            if v.engine is not eng or v.kind != REAL:
                raise ValueError("%s: a real field of this box" % name)
            return v.ptr, _FIELD, 0.0
        a = np.asarray(v, dtype=np.float64)
        if a.size == 1 and a.ndim <= 1:
            return None, _SCALAR, float(a.reshape(-1)[0])
        if a.ndim == 1 and a.size == N:
            buf = eng.upload_raw(np.ascontiguousarray(a))
            keep.append(buf)
            return buf.ptr, _ZPROFILE, 0.0
        if a.shape == (N, N, N):
            buf = eng.upload_raw(np.ascontiguousarray(a))
            keep.append(buf)
            return buf.ptr, _FIELD_F64, 0.0
        raise ValueError("%s: a scalar, a length-%d array along z or an array of shape %s" % (name, N, (N, N, N)))

    def _args(self, delta_x, nbar, bias, keep):
        box = self.box
        d = box._as_real(delta_x)
        keep.append(d)
        pn, kn, vn = self._param(nbar, "nbar", keep)
        pb, kb, vb = self._param(bias, "bias", keep)
        voxel_vol = box.Lx * box.Ly * box.Lz / box.N ** 3.
        return d.ptr, pn, kn, vn, pb, kb, vb, voxel_vol

    def expected_counts(self, delta_x, nbar, bias, lognormal=False):
        """Host fp64 (N, N, N): the expected count per voxel, lam, that halo_count_field draws from."""
        eng, N = self.box.engine, self.box.N
        keep = []
        args = self._args(delta_x, nbar, bias, keep)
        buf = eng._alloc_bytes(8 * N ** 3)
        _lib.call("fb_halo_lambda", eng._plan, *args, int(bool(lognormal)), buf.ptr, eng.stream)
        return eng.download_raw(buf, (N, N, N))

    def halo_count_field(self, delta_x, nbar, bias, lognormal=False, realisation=None):
        """Poisson halo counts per voxel (halos.py:53-117): lam = voxel_vol * nbar * (1 + delta_h), delta_h = bias * delta_x or,
        with ``lognormal``, exp(delta_h) / mean(exp(delta_h)) - 1 (formed with a shift on single-precision plans); negative lam
        is set to 0 unless log-normal, NaN to 0.  ``nbar``, ``bias``: scalar, length-N array along z (the last axis), or an
        (N, N, N) host array / DeviceArray.  Returns a real DeviceArray of integer counts.  ValueError if any lam > 2^24.
        ``realisation`` (rng='device'): the counter of the draw (default: the box's next one; kept in last_realisation)."""
        box, eng, N = self.box, self.box.engine, self.box.N
        if box.rng == "numpy":
            lam = self.expected_counts(delta_x, nbar, bias, lognormal)
            if np.max(lam) > LAM_MAX:
                raise ValueError("expected halo count above 2^24 in a voxel: counts would not be exact in fp32")
            counts = np.random.poisson(lam=lam)
            return eng.upload(counts.astype(eng.rdtype), REAL)
        keep = []
        args = self._args(delta_x, nbar, bias, keep)
        real = _next_realisation(box) if realisation is None else int(realisation)
        self.last_realisation = real
        out = eng.empty(REAL)
        over = ctypes.c_int32(0)
        _lib.call("fb_halo_counts", eng._plan, *args, int(bool(lognormal)), box.seed & (2 ** 64 - 1), real, out.ptr,
                  ctypes.byref(over), eng.stream)
        if over.value:
            raise ValueError("expected halo count above 2^24 in a voxel: counts would not be exact in fp32")
        return out

    # ------------------------------------------------------------------ catalogue
    def realise_halo_catalogue(self, Nhalo, scatter=False, scatter_type='uniform', realisation=None):
        """Halo positions (halos.py:120-176) in the reference's order: ascending count; within a count, voxels in C order,
        each repeated `count` times; pos = (index + u) * (L_a / N).  ``scatter``: u uniform on [0, 1 - 1e-8) (rng='numpy':
        np.random.uniform(0., 1.-1e-8, 3 Nh) row-major; rng='device': stream 6), else 0.  ``Nhalo``: the device counts or a
        host integer array.  Returns a HaloCatalogue (empty, shape (0, 3), for an all-zero field)."""
        box, eng, N = self.box, self.box.engine, self.box.N
        if scatter and scatter_type != 'uniform':
            raise ValueError("scatter_type='%s' not recognised" % scatter_type)
        if isinstance(Nhalo, DeviceArray):
            if Nhalo.engine is not eng or Nhalo.kind != REAL:
                raise ValueError("Nhalo: a real field of this box")
            counts = Nhalo
        else:
            a = np.asarray(Nhalo)
            if a.shape != (N, N, N):
                raise ValueError("Nhalo: expected an array of shape %s, got %s" % ((N, N, N), a.shape))
            if a.size and (np.min(a) < 0 or np.any(a != np.floor(a)) or np.max(a) > LAM_MAX):
                raise ValueError("Nhalo: non-negative integers up to 2^24")
            counts = eng.upload(a.astype(eng.rdtype), REAL)
        kt = (ctypes.c_int64 * 2)()
        _lib.call("fb_halo_catalogue_size", eng._plan, counts.ptr, kt, eng.stream)
        kmax, total = int(kt[0]), int(kt[1])
        if total == 0:
            return HaloCatalogue(eng, None, 0)
        buf = eng._alloc_bytes(24 * total)
        mode, upos, seed, real = 0, None, 0, 0
        keep = None
        if scatter:
            if box.rng == "numpy":
                u = np.random.uniform(0., 1. - 1e-8, 3 * total)
                keep = eng.upload_raw(u)
                mode, upos = 1, keep.ptr
            else:
                mode, seed = 2, box.seed & (2 ** 64 - 1)
                real = _next_realisation(box) if realisation is None else int(realisation)
                self.last_realisation = real
        _lib.call("fb_halo_catalogue", eng._plan, counts.ptr, kmax, total, upos, mode, seed, real, buf.ptr, eng.stream)
        if keep is not None:
            eng.sync()              # the host array behind the upload must outlive the copy
        return HaloCatalogue(eng, buf, total)


# ---------------------------------------------------------------------- friends-of-friends
FOF_TILE = 64                       # particles per LDS tile of the pair search (FB_FOF_TILE of fb_fof.hip)
RHO_CRIT = 2.77536627e11            # critical density today in h^2 Msun / Mpc^3


class DeviceLabels(DeviceBuffer):
    """int32 per particle on the device; ``np.asarray(labels)`` is the host copy."""

    def __init__(self, engine, buf, n):
        self.n = int(n)
        DeviceBuffer.__init__(self, engine, buf, (self.n,), np.int32)


class FoFHalos(HaloCatalogue):
    """The friends-of-friends groups of ``find_halos_fof``, largest first: a HaloCatalogue of their centres of mass (Mpc, in
    [0, L)) -- ``paint_catalogue`` takes it -- with ``count`` (members, host int64), ``mass`` (count x particle_mass, Msun),
    ``velocities`` (mean member velocity, a HaloCatalogue, or None), ``labels`` (device int32 per particle: the rank of its
    group in this catalogue, -1 if the group has fewer than nmin members), ``roots`` (least member index of each group, host
    int64), ``n_groups_all`` (groups of any size), ``linking_length`` (Mpc) and ``particle_mass`` (Msun)."""

    def __init__(self, engine, buf, n, count, roots, velocities, labels, n_groups_all, linking_length, particle_mass):
        HaloCatalogue.__init__(self, engine, buf, n)
        self.count, self.roots, self.velocities, self.labels = count, roots, velocities, labels
        self.n_groups_all, self.linking_length, self.particle_mass = int(n_groups_all), float(linking_length), float(particle_mass)
        self.mass = count.astype(np.float64) * float(particle_mass)

    def __repr__(self):
        return "FoFHalos(%d halos of %d groups, linking length %.6g Mpc)" % (self.n, self.n_groups_all, self.linking_length)


def fof_linking_length(L, n, linking_length=0.2, absolute=False):
    """The linking length in Mpc: ``linking_length`` itself, or that fraction of the mean spacing (Lx Ly Lz / n)^(1/3).
    ValueError unless 0 < l < min(L) / 2."""
    ell = float(linking_length) if absolute else float(linking_length) * (float(L[0]) * float(L[1]) * float(L[2]) / n) ** (1. / 3.)
    if not (0. < ell < 0.5 * min(L)):
        raise ValueError("linking length %.6g Mpc: must be above 0 and below half the shortest box side (%.6g Mpc)"
                         % (ell, 0.5 * min(L)))
    return ell


def fof_cells(L, ell, n):
    """Cells per axis of the pair search: side L_a / Nc_a >= l (1 + 1e-9), so that rounding in a particle's cell index cannot
    separate friends by two cells; Nc_a <= max(4, floor((n / 2)^(1/3))): two particles per cell on average in a cubic box."""
    cap = max(4, int(np.floor((0.5 * n) ** (1. / 3.))))
    return tuple(max(1, min(int(np.floor(float(La) / ell * (1. - 1e-9))), cap)) for La in L)


def fof_device_bytes(n, cells, nmin, host_positions=False, velocities=False):
    """Device bytes find_halos_fof allocates beside the particles: the link's work buffer (permuted positions, permutation,
    cell table), parents, counts, labels and the catalogue of at most n / nmin groups."""
    ncells = int(cells[0]) * int(cells[1]) * int(cells[2])
    nk = n // max(1, nmin)
    need = int(_lib.load().fb_fof_work_bytes(int(n), ncells)) + 3 * 4 * n + 8 * nk + (256 + 96 * nk) + (8 + 48) * nk + 512
    if host_positions:
        need += 24 * n * (2 if velocities else 1)
    return need


def find_halos_fof(box, particles, linking_length=0.2, nmin=20, absolute=False, particle_mass=None, velocities=None,
                   timings=None):
    """Friends-of-friends halos of a particle set on the device (nbodykit's FOF; definition and design in DESIGN.md
    section 4).  ``particles``: a ColaParticles (its velocities are used), a HaloCatalogue of this box (no velocities) or a
    host (n, 3) array in Mpc with an optional host ``velocities`` (n, 3); positions are periodic in the box and wrapped on
    read.  Two particles are friends iff their minimum-image distance is strictly below the linking length
    ``linking_length`` x (Lx Ly Lz / n)^(1/3), or ``linking_length`` Mpc with ``absolute``; groups are the connected
    components, and those of ``nmin`` members or more are returned as a ``FoFHalos``, by descending count, ties by ascending
    least member index.  ``particle_mass`` (Msun; default Omega_m 2.77536627e11 h^2 Lx Ly Lz / n, Omega_m = Omega_c + Omega_b, with lengths in Mpc, this
    package's unit -- not Mpc/h, so the mass is in Msun, not Msun/h).  ``timings``: a dict that receives the milliseconds of
    the stages.  ValueError: a bad linking length, a position or velocity that is not finite, or a position too large to wrap
    into the box (|x| >= 2^52 L); MemoryError before any
    kernel runs if the work memory does not fit; RuntimeError if a union-find loop hits its iteration cap."""
    import time
    eng = box.engine
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    nmin = int(nmin)
    if nmin < 1:
        raise ValueError("nmin must be >= 1")
    keep = []
    host = not isinstance(particles, HaloCatalogue)
    if not host:
        if particles.engine is not eng:
            raise ValueError("particles: a catalogue of this box")
        if velocities is not None:
            raise ValueError("velocities: only with host positions (a ColaParticles carries its own)")
        n = particles.n
        vcat = getattr(particles, "velocities", None)
        vcat = vcat if isinstance(vcat, HaloCatalogue) and vcat.n == n else None
    else:
        p = np.ascontiguousarray(particles, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("particles: an (n, 3) array")
        n = p.shape[0]
        v = None
        if velocities is not None:
            v = np.ascontiguousarray(velocities, dtype=np.float64)
            if v.shape != p.shape:
                raise ValueError("velocities: expected shape %s, got %s" % (p.shape, v.shape))
    if n > 2 ** 31 - 2:
        raise ValueError("friends-of-friends: at most 2^31 - 2 particles")
    ell = fof_linking_length(L, n, linking_length, absolute) if (n or absolute) else float("nan")
    pmass = float(particle_mass) if particle_mass is not None else \
        ((box.cosmo['Omega_c'] + box.cosmo['Omega_b']) * RHO_CRIT * box.cosmo['h'] ** 2 * L[0] * L[1] * L[2] / n if n else 0.)
    has_vel = (v is not None) if host else (vcat is not None)

    def empty(ngroups, labels):
        vel = HaloCatalogue(eng, None, 0) if has_vel else None
        return FoFHalos(eng, None, 0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), vel, labels, ngroups, ell, pmass)

    if n == 0:
        return empty(0, DeviceLabels(eng, None, 0))
    cells = fof_cells(L, ell, n)
    eng.need_memory(fof_device_bytes(n, cells, nmin, host, has_vel),
                    "find_halos_fof: %d particles in %d x %d x %d cells take" % ((n,) + cells))
    if host:
        pbuf = eng.upload_raw(p)
        keep.append(pbuf)
        pptr, vptr = pbuf.ptr, None
        if v is not None:
            vbuf = eng.upload_raw(v)
            keep.append(vbuf)
            vptr = vbuf.ptr
    else:
        pptr, vptr = particles.ptr, (vcat.ptr if vcat is not None else None)
    try:
        # 1-3. cells, pair search with union-find, flattening: the root of every particle
        wbytes = int(eng.lib.fb_fof_work_bytes(n, cells[0] * cells[1] * cells[2]))
        work, root = eng._alloc_bytes(wbytes), eng._alloc_bytes(4 * n)
        bad = ctypes.c_int32(0)
        nc = (ctypes.c_int32 * 3)(*cells)
        ms = (ctypes.c_double * 4)()
        _lib.call("fb_fof_link", eng._plan, pptr, n, ell, nc, work.ptr, wbytes, root.ptr, ctypes.byref(bad),
                  ms if timings is not None else None, eng.stream)
        if bad.value:
            raise ValueError("find_halos_fof: a position is not finite, or too large to wrap into the box")
        del work
        t0 = time.perf_counter()
        # 4. sizes; the (count, root) order of the groups kept is formed on the host
        cap = n // nmin
        count, small = eng._alloc_bytes(4 * n), eng._alloc_bytes(256)
        kept = eng._alloc_bytes(8 * cap) if cap else None
        out = (ctypes.c_int64 * 2)()
        _lib.call("fb_fof_sizes", eng._plan, root.ptr, n, nmin, small.ptr, count.ptr, kept.ptr if cap else None, out, eng.stream)
        ngroups, nk = int(out[0]), int(out[1])
        del count
        pairs = eng.download_raw(kept, (nk, 2), np.uint32)
        del kept
        order = np.lexsort((pairs[:, 0], -pairs[:, 1].astype(np.int64)))
        sroots, scounts = np.ascontiguousarray(pairs[order, 0]), np.ascontiguousarray(pairs[order, 1])
        labels = eng._alloc_bytes(4 * n)
        cbuf = vout = None
        if nk:
            keep.extend([eng.upload_raw(sroots), eng.upload_raw(scounts)])
            cbuf = eng._alloc_bytes(24 * nk)
            vout = eng._alloc_bytes(24 * nk) if has_vel else None
            cwork = eng._alloc_bytes(256 + 96 * nk)
            args = (keep[-2].ptr, keep[-1].ptr, nk, cwork.ptr)
        else:
            args = (None, None, 0, None)
        _lib.call("fb_fof_catalogue", eng._plan, pptr, vptr, root.ptr, n, *args, labels.ptr, cbuf.ptr if nk else None,
                  vout.ptr if vout is not None else None, ctypes.byref(bad), eng.stream)
        eng.sync()                          # host arrays behind the uploads must outlive the copies
        if bad.value:
            raise ValueError("find_halos_fof: a velocity is not finite, or n max |v| overflows")
    except _lib.FastBoxError as e:
        if e.code == -5:                    # FB_ERR_STATE: an iteration cap
            raise RuntimeError("find_halos_fof: %s" % e)
        raise
    if timings is not None:
        timings.update(bin_ms=ms[0], link_ms=ms[1] + ms[2], link_crowded_ms=ms[2], flatten_ms=ms[3], catalogue_ms=1e3 * (time.perf_counter() - t0),
                       cells=cells)
    lab = DeviceLabels(eng, labels, n)
    if not nk:
        return empty(ngroups, lab)
    vel = HaloCatalogue(eng, vout, nk) if has_vel else None
    return FoFHalos(eng, cbuf, nk, scounts.astype(np.int64), sroots.astype(np.int64), vel, lab, ngroups, ell, pmass)



# ---------------------------------------------------------------------- pair counts
PAIR_MODES = {"1d": 0, "2d": 1, "projected": 2}
PAIR_MAX_NR, PAIR_MAX_BINS = 256, 4096          # FB_PAIR_MAX_NR, FB_PAIR_MAX_BINS of fb_pairs.hip
_LEGENDRE = {0: lambda m: np.ones_like(m), 2: lambda m: 0.5 * (3. * m * m - 1.), 4: lambda m: 0.125 * ((35. * m * m - 30.) * m * m + 3.)}


class PairCounts(object):
    """Pair counts of one or two catalogues in the periodic box and the natural estimator with analytic RR on top of them
    (``pair_counts``).  Members: ``mode``; ``edges`` (r edges, or r_p edges for 'projected', Mpc);
    ``r``, the arithmetic bin midpoints; ``mu_edges`` ('2d') or ``pi_edges`` ('projected'), else None; ``npairs`` int64 of
    shape (nr,), (nr, Nmu) or (nr, npi): ordered pairs, so every auto count is even; ``rr`` = P V_bin / (Lx Ly Lz), P =
    n (n - 1) for auto-counts and n1 n2 for cross-counts, V_bin = (4 pi / 3)(r1^3 - r0^3), times dmu for '2d', and
    pi (r_p1^2 - r_p0^2) 2 dpi for 'projected'; ``xi`` = npairs / rr - 1 (NaN where rr = 0: an empty catalogue); ``poles``, a
    dict l -> xi_l(r) = (2 l + 1) sum_m xi(r, mu_m) P_l(mu_m) dmu at the mu midpoints ('2d' with ``poles``; else {});
    ``wp`` = 2 sum_pi xi(r_p, pi) dpi ('projected'; else None); ``n1``, ``n2``, ``auto``."""

    def __init__(self, edges, npairs, L, n1, n2, auto, mode='1d', poles=None):
        self.mode = mode
        self.edges = np.array(edges, dtype=np.float64)
        self.npairs = np.array(npairs, dtype=np.int64)
        self.n1, self.n2, self.auto = int(n1), int(n2), bool(auto)
        self.L = tuple(float(a) for a in L)
        e = self.edges
        nr = e.size - 1
        if mode not in PAIR_MODES or self.npairs.ndim != (1 if mode == '1d' else 2) or self.npairs.shape[0] != nr:
            raise ValueError("PairCounts: counts of shape (nr,) for '1d', (nr, nsub) for '2d' and 'projected'")
        self.r = 0.5 * (e[1:] + e[:-1])
        self.mu_edges = self.pi_edges = self.wp = None
        P = float(self.n1) * float(self.n1 - 1) if self.auto else float(self.n1) * float(self.n2)
        box_volume = self.L[0] * self.L[1] * self.L[2]
        if mode == 'projected':
            npi = self.npairs.shape[1]
            self.pi_edges = np.arange(npi + 1, dtype=np.float64)
            vol = (np.pi * (e[1:] ** 2 - e[:-1] ** 2))[:, None] * (2. * np.diff(self.pi_edges))[None, :]
        else:
            vol = (4. * np.pi / 3.) * (e[1:] ** 3 - e[:-1] ** 3)
            if mode == '2d':
                nmu = self.npairs.shape[1]
                self.mu_edges = np.arange(nmu + 1, dtype=np.float64) / nmu
                vol = vol[:, None] * np.diff(self.mu_edges)[None, :]
        self.rr = P * vol / box_volume
        with np.errstate(divide='ignore', invalid='ignore'):
            self.xi = np.where(self.rr > 0., self.npairs / self.rr - 1., np.nan)
        self.poles = {}
        if poles is not None:
            if mode != '2d':
                raise ValueError("poles: with mode='2d' only")
            mu = 0.5 * (self.mu_edges[1:] + self.mu_edges[:-1])
            dmu = np.diff(self.mu_edges)
            for l in _check_pair_poles(poles):
                self.poles[l] = (2 * l + 1) * np.sum(self.xi * (_LEGENDRE[l](mu) * dmu)[None, :], axis=1)
        if mode == 'projected':
            self.wp = 2. * np.sum(self.xi * np.diff(self.pi_edges)[None, :], axis=1)

    def __repr__(self):
        return "PairCounts(%s, %s, n1=%d, n2=%d, bins %s)" % (self.mode, "auto" if self.auto else "cross", self.n1, self.n2,
                                                             self.npairs.shape)


def _check_pair_poles(poles):
    ps = tuple(int(l) for l in poles)
    if not ps or any(l not in (0, 2, 4) for l in ps) or len(set(ps)) != len(ps):
        raise ValueError("poles: a subset of (0, 2, 4)")
    return ps


def pair_setup(L, N, edges=None, mode='1d', Nmu=10, pimax=None, poles=None):
    """The checked arguments of ``pair_counts`` as (edges, nsub, sub_max, reach): nsub = 1, Nmu or int(pimax); reach = the
    largest separation along each axis.  Default edges: 20 logarithmic bins from min(L) / N, one cell of the box's grid, to
    min(L) / 8 (the minimum over x and y only for 'projected'); they exist for N > 8 only.  ValueError for anything ``pair_counts`` does not accept."""
    L = tuple(float(a) for a in L)
    if mode not in PAIR_MODES:
        raise ValueError("mode must be one of %s" % sorted(PAIR_MODES))
    if poles is not None:
        if mode != '2d':
            raise ValueError("poles: with mode='2d' only")
        _check_pair_poles(poles)
    if pimax is not None and mode != 'projected':
        raise ValueError("pimax: with mode='projected' only")
    lmin = min(L[:2]) if mode == 'projected' else min(L)
    if edges is None:
        if int(N) <= 8:
            raise ValueError("edges: the default (min(L) / N to min(L) / 8) needs a box of N > 8 cells per side; pass edges")
        edges = np.geomspace(lmin / int(N), lmin / 8., 21)
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or not np.all(np.isfinite(e)) or e[0] < 0. or not np.all(e[1:] > e[:-1]):
        raise ValueError("edges: a strictly ascending array of at least 2 finite values, edges[0] >= 0")
    nr = e.size - 1
    if nr > PAIR_MAX_NR:
        raise ValueError("edges: at most %d bins, got %d" % (PAIR_MAX_NR, nr))
    if not e[-1] < 0.5 * lmin:
        raise ValueError("edges: the last edge %.6g Mpc must be below half the shortest box side%s (%.6g Mpc)"
                         % (e[-1], " across the line of sight" if mode == 'projected' else "", 0.5 * lmin))
    nsub, sub_max, reach = 1, 0., (e[-1],) * 3
    if mode == '2d':
        if int(Nmu) != Nmu or int(Nmu) < 1:
            raise ValueError("Nmu: a positive integer")
        nsub = int(Nmu)
    elif mode == 'projected':
        if pimax is None or not np.isfinite(pimax) or pimax <= 0. or int(pimax) != pimax:
            raise ValueError("pimax: a positive integer value in Mpc (one pi bin per Mpc)")
        if not pimax < 0.5 * L[2]:
            raise ValueError("pimax: %.6g Mpc must be below half the box side along the line of sight (%.6g Mpc)" % (pimax, 0.5 * L[2]))
        nsub, sub_max = int(pimax), float(pimax)
        reach = (e[-1], e[-1], sub_max)
    if nr * nsub > PAIR_MAX_BINS:
        raise ValueError("%d x %d bins: at most %d bins in total (and at most %d in r)" % (nr, nsub, PAIR_MAX_BINS, PAIR_MAX_NR))
    return e, nsub, sub_max, reach


def pair_cells(L, reach, n):
    """Cells per axis of the pair sweep: side L_a / Nc_a >= reach_a (1 + 1e-9) as ``fof_cells`` has it, at least 2 per axis
    (reach_a < L_a / 2; with 2 or 3 cells every cell is a neighbour, so the margin is not needed there) and at most
    max(4, floor((n / 2)^(1/3)))."""
    cap = max(4, int(np.floor((0.5 * n) ** (1. / 3.))))
    return tuple(max(2, min(int(np.floor(float(La) / float(ra) * (1. - 1e-9))), cap)) for La, ra in zip(L, reach))


def pair_device_bytes(n1, n2, cells, nbins=PAIR_MAX_BINS, host_first=False, host_second=False):
    """Device bytes pair_counts allocates beside the catalogues: the work buffer (permuted positions, cell ids and cell
    tables of both catalogues -- ``n2`` = 0 for auto-counts), the counts, and the uploads of host positions."""
    ncells = int(cells[0]) * int(cells[1]) * int(cells[2])
    need = int(_lib.load().fb_pair_work_bytes(int(n1), int(n2), ncells)) + 8 * int(nbins) + 512
    return need + (24 * n1 + 32 if host_first else 0) + (24 * n2 + 32 if host_second else 0)


def _pair_positions(eng, x, name):
    """(n, host array or None, catalogue or None) of one input of pair_counts."""
    if isinstance(x, HaloCatalogue):
        if x.engine is not eng:
            raise ValueError("%s: a catalogue of this box" % name)
        return x.n, None, x
    p = np.ascontiguousarray(x, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("%s: an (n, 3) array" % name)
    return p.shape[0], p, None


def pair_counts(box, first, second=None, edges=None, mode='1d', Nmu=10, pimax=None, poles=None, timings=None):
    """Pair counts in separation bins on the device, and the correlation function from them (nbodykit's
    ``SimulationBox2PCF``; definition and design in DESIGN.md section 4).  ``first``, ``second``: a HaloCatalogue of this box
    (FoFHalos, ColaParticles) or a host (n, 3) array in Mpc; positions are periodic in the box and wrapped on read, as in
    ``find_halos_fof``.  ``second`` None, or the same object as ``first``: auto-counts (ordered pairs i != j); anything else,
    a separate copy of the same positions included: cross-counts (all n1 n2 pairs).  ``mode``: '1d' bins in r; '2d' in
    (r, mu), mu = |dz| / r in ``Nmu`` uniform bins (a pair at d = 0 goes to the last one); 'projected' in (r_p, pi), pi = |dz|
    in int(pimax) bins of 1 Mpc -- the line of sight is z.  ``edges``: r (or r_p) edges in Mpc, lower edge inclusive, upper
    exclusive, decided on squares; default and limits: ``pair_setup``.  ``poles``: a subset of (0, 2, 4), '2d' only.
    ``timings``: a dict that receives the milliseconds of the stages.  Returns a ``PairCounts``.  ValueError: bad arguments
    (before the device is touched), a position that is not finite or too large to wrap into the box (|x| >= 2^52 L);
    MemoryError before any kernel runs if the work memory does not fit."""
    eng = box.engine
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    e, nsub, sub_max, reach = pair_setup(L, getattr(box, "N", 1), edges, mode, Nmu, pimax, poles)
    auto = second is None or second is first
    n1, h1, c1 = _pair_positions(eng, first, "first")
    n2, h2, c2 = (n1, None, None) if auto else _pair_positions(eng, second, "second")
    if max(n1, n2) > 2 ** 31 - 2:
        raise ValueError("pair counts: at most 2^31 - 2 particles in a catalogue")
    nr = e.size - 1
    nbins = nr * nsub
    cells = pair_cells(L, reach, max(n1, n2, 1))
    eng.need_memory(pair_device_bytes(n1, 0 if auto else n2, cells, nbins, h1 is not None, h2 is not None),
                    "pair_counts: %d and %d particles in %d x %d x %d cells take" % ((n1, n2) + cells))
    keep = []

    def pointer(n, host, cat):
        if n == 0:                      # an empty catalogue still needs an address: NULL means auto-counts
            keep.append(eng._alloc_bytes(32))
            return keep[-1].ptr
        if cat is not None:
            return cat.ptr
        keep.append(eng.upload_raw(host))
        return keep[-1].ptr

    p1 = pointer(n1, h1, c1)
    p2 = None if auto else pointer(n2, h2, c2)
    wbytes = int(eng.lib.fb_pair_work_bytes(n1, 0 if auto else n2, cells[0] * cells[1] * cells[2]))
    work, out = eng._alloc_bytes(wbytes), eng._alloc_bytes(8 * nbins)
    e2 = np.ascontiguousarray(e * e)
    bad = ctypes.c_int32(0)
    nc = (ctypes.c_int32 * 3)(*cells)
    ms = (ctypes.c_double * 3)()
    _lib.call("fb_pair_count", eng._plan, p1, n1, p2, 0 if auto else n2, PAIR_MODES[mode],
              e2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nr, nsub, sub_max, nc, work.ptr, wbytes, out.ptr, ctypes.byref(bad),
              ms if timings is not None else None, eng.stream)
    if bad.value:
        raise ValueError("pair_counts: a position is not finite, or too large to wrap into the box")
    counts = eng.download_raw(out, nbins, np.uint64)        # (waits: the host arrays behind the uploads outlive the copies)
    if timings is not None:
        timings.update(bin_ms=ms[0], count_ms=ms[1] + ms[2], count_crowded_ms=ms[2], cells=cells)
    npairs = counts.astype(np.int64).reshape((nr,) if mode == '1d' else (nr, nsub))
    return PairCounts(e, npairs, L, n1, n2, auto, mode=mode, poles=poles)


# ---------------------------------------------------------------------- radial profiles and spherical-overdensity masses
PROFILE_MAX_NR = 256                # FB_PROF_MAX_NR of fb_profiles.hip
SO_RMAX = 5.                        # Mpc: the default outer edge of spherical_overdensity


class HaloProfiles(object):
    """Radial profiles of all particles around given centres (``halo_profiles``).  Members: ``edges``
    (nr + 1, Mpc); ``r``, the arithmetic bin midpoints; ``counts`` int64 (nh, nr): particles with edges[b]^2 <= d^2 <
    edges[b + 1]^2; ``inner`` int64 (nh,): particles with d^2 < edges[0]^2; ``enclosed`` int64 (nh, nr + 1): N(< edges[j]) =
    inner + sum_{b < j} counts; ``density`` (nh, nr): particle_mass counts / (4 pi / 3 (e1^3 - e0^3)), Msun / Mpc^3;
    ``enclosed_density`` (nh, nr + 1): particle_mass N(< e_j) / (4 pi / 3 e_j^3), NaN at an edge of 0; ``particle_mass``."""

    def __init__(self, edges, inner, counts, particle_mass):
        self.edges = np.array(edges, dtype=np.float64)
        self.inner = np.array(inner, dtype=np.int64)
        self.counts = np.array(counts, dtype=np.int64).reshape(self.inner.size, self.edges.size - 1)
        self.particle_mass = float(particle_mass)
        e = self.edges
        self.r = 0.5 * (e[1:] + e[:-1])
        self.enclosed = np.concatenate([self.inner[:, None], self.inner[:, None] + np.cumsum(self.counts, axis=1)], axis=1)
        self.density = self.particle_mass * self.counts / ((4. * np.pi / 3.) * (e[1:] ** 3 - e[:-1] ** 3))[None, :]
        with np.errstate(divide='ignore', invalid='ignore'):
            self.enclosed_density = np.where(e > 0., self.particle_mass * self.enclosed / ((4. * np.pi / 3.) * e ** 3)[None, :], np.nan)

    def __len__(self):
        return self.inner.size

    def __repr__(self):
        return "HaloProfiles(%d centres, %d bins)" % (self.inner.size, self.edges.size - 1)


class SOHalos(HaloCatalogue):
    """The spherical-overdensity halos of ``spherical_overdensity``: a HaloCatalogue whose positions are the input centres
    -- ``paint_catalogue`` and ``pair_counts`` take it -- with, per centre, ``radius`` (R_Delta, Mpc), ``mass`` (M_Delta =
    4 pi / 3 Delta rho_ref R^3, Msun) and ``status`` (0: found; 1: nowhere above the threshold; 2: still above it at the last
    edge; radius and mass are NaN unless 0), ``count`` (int64: the particles with d^2 < R^2 exactly; 0 unless status 0),
    ``com`` (a HaloCatalogue: their centre of mass, NaN where count is 0), ``velocities`` (a HaloCatalogue of their mean
    velocity) and ``sigma_v`` (host, km/s: the 1-d dispersion), both None without particle velocities, ``profiles`` (the
    ``HaloProfiles`` behind the radii), ``delta``, ``rho_ref`` (comoving Msun / Mpc^3) and ``particle_mass``."""

    def __init__(self, engine, buf, n, radius, mass, status, count, com, velocities, sigma_v, profiles, delta, rho_ref):
        HaloCatalogue.__init__(self, engine, buf, n)
        self.radius, self.mass, self.status, self.count = radius, mass, status, count
        self.com, self.velocities, self.sigma_v, self.profiles = com, velocities, sigma_v, profiles
        self.delta, self.rho_ref, self.particle_mass = float(delta), float(rho_ref), profiles.particle_mass

    def __repr__(self):
        return "SOHalos(%d centres, %d with a radius, Delta = %g)" % (self.n, int(np.count_nonzero(self.status == 0)), self.delta)


def so_reference_density(box, reference='mean'):
    """rho_ref of ``spherical_overdensity``, comoving, in Msun / Mpc^3: 'mean': Omega_m 2.77536627e11 h^2; 'crit': the
    critical density at the box redshift, 2.77536627e11 h^2 E(a)^2 a^3; or a positive number, taken as it is."""
    h2 = float(box.cosmo['h']) ** 2
    if isinstance(reference, str):
        if reference == 'mean':
            return (box.cosmo['Omega_c'] + box.cosmo['Omega_b']) * RHO_CRIT * h2
        if reference == 'crit':
            from .box import _ccl
            a = float(box.scale_factor)
            return RHO_CRIT * h2 * float(_ccl.h_over_h0(box.cosmo, a)) ** 2 * a ** 3
        raise ValueError("reference: 'mean', 'crit' or a density in Msun / Mpc^3")
    rho = float(reference)
    if not (np.isfinite(rho) and rho > 0.):
        raise ValueError("reference: 'mean', 'crit' or a positive density in Msun / Mpc^3")
    return rho


def so_from_enclosed(edges, enclosed, particle_mass, rho_ref, delta):
    """(radius, mass, status) from enclosed counts: pure numpy, no device.  ``enclosed`` (nh, nr + 1): N(< edges[j]).
    rho_j = particle_mass N(< e_j) / (4 pi / 3 e_j^3) at every edge e_j > 0; j* = the largest j with rho_j >= delta rho_ref
    -- the outermost crossing, on purpose: a single inner bin with one particle is noisy, and the first down-crossing stops
    there.  status 1: no such j; 2: j* is the last edge; both give NaN.  status 0: R is the log-log linear interpolation of
    (e, rho) between j* and j* + 1 at rho = delta rho_ref, and M = 4 pi / 3 delta rho_ref R^3."""
    e = np.asarray(edges, dtype=np.float64)
    N = np.asarray(enclosed, dtype=np.float64).reshape(-1, e.size)
    nh, nr = N.shape[0], e.size - 1
    thr = float(delta) * float(rho_ref)
    pos = e > 0.
    rho = np.zeros_like(N)
    rho[:, pos] = float(particle_mass) * N[:, pos] / ((4. * np.pi / 3.) * e[pos] ** 3)[None, :]
    above = (rho >= thr) & pos[None, :]
    any_above = above.any(axis=1)
    jstar = nr - np.argmax(above[:, ::-1], axis=1)                    # the last True of each row (meaningless without one)
    status = np.where(~any_above, 1, np.where(jstar == nr, 2, 0)).astype(np.int64)
    radius = np.full(nh, np.nan)
    ok = np.nonzero(status == 0)[0]
    if ok.size:
        j = jstar[ok]
        le0, le1 = np.log(e[j]), np.log(e[j + 1])
        lr0, lr1 = np.log(rho[ok, j]), np.log(rho[ok, j + 1])         # rho_j >= thr > rho_{j + 1} > 0: N does not decrease
        radius[ok] = np.clip(np.exp(le0 + (np.log(thr) - lr0) * (le1 - le0) / (lr1 - lr0)), e[j], e[j + 1])   # rounding stays inside
    mass = (4. * np.pi / 3.) * thr * radius ** 3
    return radius, mass, status


def profile_edges(L, edges):
    """The checked radial edges of ``halo_profiles``: strictly ascending, finite, edges[0] >= 0, at most 256 bins, the last
    edge below min(L) / 2.  ValueError otherwise."""
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or not np.all(np.isfinite(e)) or e[0] < 0. or not np.all(e[1:] > e[:-1]):
        raise ValueError("edges: a strictly ascending array of at least 2 finite values, edges[0] >= 0")
    if e.size - 1 > PROFILE_MAX_NR:
        raise ValueError("edges: at most %d bins, got %d" % (PROFILE_MAX_NR, e.size - 1))
    if not e[-1] < 0.5 * min(L):
        raise ValueError("edges: the last edge %.6g Mpc must be below half the shortest box side (%.6g Mpc)" % (e[-1], 0.5 * min(L)))
    return e


def profile_device_bytes(n, nh, cells, nr=PROFILE_MAX_NR, velocities=False, host_particles=False, host_centres=False):
    """Device bytes halo_profiles and spherical_overdensity allocate beside the particles and centres: the work buffer (28
    bytes a particle -- the permuted positions and cell ids -- and 28 more with velocities: their permuted copy and the
    permutation), the (nh, nr + 1) counts, the aperture outputs (radii, counts, centres of mass, mean velocities,
    dispersions) and the uploads of host inputs."""
    ncells = int(cells[0]) * int(cells[1]) * int(cells[2])
    need = int(_lib.load().fb_profile_work_bytes(int(n), ncells, 1 if velocities else 0)) + 4 * nh * (nr + 1) + (8 + 4 + 24 + 24 + 8) * nh + 512
    if host_particles:
        need += (24 * n + 32) * (2 if velocities else 1)
    return need + (24 * nh + 32 if host_centres else 0)


class _CentreSweeps(object):
    """The particles of one call binned once on the device (fb_profile_bin), for the profile sweep and the aperture sweep."""

    def __init__(self, box, who, centres, particles, velocities, reach, nr, timings):
        import time
        self.eng = eng = box.engine
        self.who, self.timings, self.time = who, timings, time
        self.L = L = (float(box.Lx), float(box.Ly), float(box.Lz))
        self.keep = keep = []
        self.nh, hc, cc = _pair_positions(eng, centres, "centres")
        vhost = vcat = None
        if isinstance(particles, HaloCatalogue):
            if particles.engine is not eng:
                raise ValueError("particles: a catalogue of this box")
            if velocities is not None:
                raise ValueError("velocities: only with host positions (a ColaParticles carries its own)")
            self.n, hp = particles.n, None
            vcat = getattr(particles, "velocities", None)
            vcat = vcat if isinstance(vcat, HaloCatalogue) and vcat.n == self.n else None
        else:
            hp = np.ascontiguousarray(particles, dtype=np.float64)
            if hp.ndim != 2 or hp.shape[1] != 3:
                raise ValueError("particles: an (n, 3) array")
            self.n = hp.shape[0]
            if velocities is not None:
                vhost = np.ascontiguousarray(velocities, dtype=np.float64)
                if vhost.shape != hp.shape:
                    raise ValueError("velocities: expected shape %s, got %s" % (hp.shape, vhost.shape))
        n, nh = self.n, self.nh
        if max(n, nh) > 2 ** 31 - 2:
            raise ValueError("%s: at most 2^31 - 2 particles and as many centres" % who)
        self.has_vel = vhost is not None or vcat is not None
        self.reach = float(reach)
        self.cells = cells = pair_cells(L, (self.reach,) * 3, max(n, 1))
        eng.need_memory(profile_device_bytes(n, nh, cells, nr, self.has_vel, hp is not None, hc is not None),
                        "%s: %d particles in %d x %d x %d cells and %d centres take" % ((who, n) + cells + (nh,)))

        def pointer(m, host, cat):
            if m == 0:
                return None, None
            if cat is not None:
                return cat.ptr, cat._buf
            keep.append(eng.upload_raw(host))
            return keep[-1].ptr, keep[-1]

        self.cptr, self.cbuf = pointer(nh, hc, cc)
        pptr, _ = pointer(n, hp, particles if hp is None else None)
        vptr, _ = pointer(n if self.has_vel else 0, vhost, vcat)
        self.wbytes = int(eng.lib.fb_profile_work_bytes(n, cells[0] * cells[1] * cells[2], 1 if self.has_vel else 0))
        self.work = eng._alloc_bytes(self.wbytes)
        bad = ctypes.c_int32(0)
        ms = (ctypes.c_double * 1)()
        # (with no particle there is no velocity array to point to, and no velocity to check)
        _lib.call("fb_profile_bin", eng._plan, pptr, n, vptr, (ctypes.c_int32 * 3)(*cells), self.work.ptr, self.wbytes,
                  ctypes.byref(bad), ms if timings is not None else None, eng.stream)
        eng.sync()                          # host arrays behind the uploads must outlive the copies
        self.binned_vel = self.has_vel and n > 0
        if bad.value & 1:
            raise ValueError("%s: a position is not finite, or too large to wrap into the box" % who)
        if bad.value:
            raise ValueError("%s: a velocity is not finite, or n max |v|^2 overflows" % who)
        if timings is not None:
            timings.update(bin_ms=ms[0], cells=cells)

    def _bad(self, bad):
        if bad.value & 1:
            raise ValueError("%s: a centre is not finite, or too large to wrap into the box" % self.who)
        if bad.value:
            raise ValueError("%s: an aperture beyond the reach of the cells" % self.who)

    def profiles(self, e):
        """(nh, nr + 1) int64: column 0 the particles inside edges[0], then the bins."""
        eng, nh, ncol = self.eng, self.nh, e.size
        rows = np.zeros((nh, ncol), dtype=np.uint32)
        if nh:
            t0 = self.time.perf_counter()
            out = eng._alloc_bytes(rows.nbytes)
            e2 = np.ascontiguousarray(e * e)
            bad = ctypes.c_int32(0)
            _lib.call("fb_halo_profiles", eng._plan, self.work.ptr, self.cptr, nh, e2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                      ncol - 1, out.ptr, ctypes.byref(bad), eng.stream)
            self._bad(bad)
            if self.timings is not None:
                self.timings["profile_ms"] = 1e3 * (self.time.perf_counter() - t0)
            rows = eng.download_raw(out, rows.shape, np.uint32)
        return rows.astype(np.int64)

    def apertures(self, r2):
        """(count int64 (nh,), com buffer, vmean buffer or None, sigma (nh,) or None) of the particles with d^2 < r2."""
        eng, nh = self.eng, self.nh
        vel = self.has_vel
        if not nh:
            return np.zeros(0, dtype=np.int64), None, None, (np.zeros(0) if vel else None)
        r2 = np.ascontiguousarray(r2, dtype=np.float64)
        rbuf = eng.upload_raw(r2)
        cnt, com = eng._alloc_bytes(4 * nh), eng._alloc_bytes(24 * nh)
        vm = eng._alloc_bytes(24 * nh) if vel else None
        sg = eng._alloc_bytes(8 * nh) if vel else None
        dev_vel = self.binned_vel
        bad = ctypes.c_int32(0)
        t0 = self.time.perf_counter()
        _lib.call("fb_halo_apertures", eng._plan, self.work.ptr, self.cptr, rbuf.ptr, nh, self.reach, cnt.ptr, com.ptr,
                  vm.ptr if dev_vel else None, sg.ptr if dev_vel else None, ctypes.byref(bad), eng.stream)
        self._bad(bad)
        if self.timings is not None:
            self.timings["aperture_ms"] = 1e3 * (self.time.perf_counter() - t0)
        count = eng.download_raw(cnt, nh, np.uint32)
        sigma = None
        if vel:
            if dev_vel:
                sigma = eng.download_raw(sg, nh)
            else:                           # velocities of no particle: every mean is NaN
                sigma = np.full(nh, np.nan)
                nanv = np.full((nh, 3), np.nan)
                _lib.call("fb_memcpy_h2d", vm.ptr, nanv.ctypes.data_as(ctypes.c_void_p), nanv.nbytes, eng.stream)
        eng.sync()
        return count.astype(np.int64), com, vm, sigma


def _profile_mass(box, n, particle_mass):
    if particle_mass is not None:
        return float(particle_mass)
    return (box.cosmo['Omega_c'] + box.cosmo['Omega_b']) * RHO_CRIT * box.cosmo['h'] ** 2 * float(box.Lx) * float(box.Ly) * float(box.Lz) / n \
        if n else 0.


def halo_profiles(box, centres, particles, edges, particle_mass=None, timings=None):
    """Radial profiles of the particles around given centres, counted on the device (definition and design in DESIGN.md
    section 4).  ``centres``: a FoFHalos or other HaloCatalogue of this box, or a host (nh, 3) array; ``particles``: as for
    ``find_halos_fof``.  Positions are periodic in the box and wrapped on read; d^2 = (dx dx + dy dy) + dz dz on the
    minimum-image differences.  All particles count, whatever group they belong to, a particle on the centre included.
    ``edges``: radial edges in Mpc, lower edge inclusive, upper exclusive, decided on squares (``profile_edges``).
    ``particle_mass``: Msun, default that of ``find_halos_fof``.  ``timings``: a dict that receives the milliseconds of the
    stages.  Returns a ``HaloProfiles``.  ValueError: bad edges (before the device is touched), a position or centre that is
    not finite or too large to wrap into the box (|x| >= 2^52 L); MemoryError before any kernel runs if the work memory does
    not fit."""
    e = profile_edges((float(box.Lx), float(box.Ly), float(box.Lz)), edges)
    sw = _CentreSweeps(box, "halo_profiles", centres, particles, None, e[-1], e.size - 1, timings)
    rows = sw.profiles(e)
    return HaloProfiles(e, rows[:, 0], rows[:, 1:], _profile_mass(box, sw.n, particle_mass))


def halo_apertures(box, centres, particles, radius2, velocities=None, timings=None):
    """Moments of the particles inside each centre's own sphere, summed on the device: ``radius2`` (nh,) holds the *squared*
    radii in Mpc^2, a particle is a member iff d^2 < radius2 strictly (so a radius of 0 has no member).  Returns host arrays
    (count int64 (nh,), com (nh, 3), vmean (nh, 3) or None, sigma_v (nh,) or None): com = wrap(c + sum d / m), vmean =
    sum v / m, sigma_v = sqrt(max(0, (sum v.v / m - vmean.vmean) / 3)), NaN where m = 0.  The sums are fixed-point: the same
    bit for bit from call to call and for any order of the particles.  Inputs and errors as ``halo_profiles``; the largest
    radius must stay below min(L) / 2."""
    r2 = np.ascontiguousarray(radius2, dtype=np.float64).reshape(-1)
    nh = centres.n if isinstance(centres, HaloCatalogue) else np.shape(centres)[0]
    if r2.size != nh or not np.all(np.isfinite(r2)) or np.any(r2 < 0.):
        raise ValueError("radius2: %d finite squared radii >= 0" % nh)
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    reach = float(np.sqrt(r2.max())) * (1. + 1e-15) if nh else 0.
    reach = max(reach, 1e-3 * min(L))                    # cells no finer than a thousandth of the box
    if not reach < 0.5 * min(L):
        raise ValueError("radius2: the largest radius %.6g Mpc must be below half the shortest box side (%.6g Mpc)" % (reach, 0.5 * min(L)))
    sw = _CentreSweeps(box, "halo_apertures", centres, particles, velocities, reach, 0, timings)
    count, com, vm, sigma = sw.apertures(r2)
    return count, np.array(HaloCatalogue(sw.eng, com, nh)), (np.array(HaloCatalogue(sw.eng, vm, nh)) if sw.has_vel else None), sigma


def spherical_overdensity(box, centres, particles, delta=200., reference='mean', rmax=None, nbins=32, rmin=None, edges=None,
                          particle_mass=None, velocities=None, timings=None):
    """Spherical-overdensity radii and masses around given centres (definition, design and the differences from nbodykit's
    conventions in DESIGN.md section 4): the profile of all particles around every centre (``halo_profiles``), R_Delta where
    the mean enclosed density falls through ``delta`` x rho_ref for the last time (``so_from_enclosed``), M_Delta = 4 pi / 3
    delta rho_ref R^3, and one more sweep for the particles with d^2 < R^2 exactly: their number, centre of mass, mean
    velocity and velocity dispersion.  The particles are binned once for both sweeps.  ``reference``: 'mean', 'crit' or a
    density (``so_reference_density``).  ``edges``: radial edges in Mpc; default ``nbins`` logarithmic bins from ``rmin``
    (default a quarter of the mean particle spacing, at most rmax / 2) to ``rmax`` (default 5 Mpc -- beyond the virial radius
    of any cluster -- or 0.45 min(L) in a box too small for that).  A centre still above the threshold at the last edge gets
    status 2: pass a larger ``rmax``.  ``velocities``: host (n, 3), with host particles only; a ColaParticles brings its own.
    No unbinding, no recentring.  Returns an ``SOHalos``.  Errors: as ``halo_profiles``, and ValueError for a velocity that is
    not finite."""
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    delta = float(delta)
    if not (np.isfinite(delta) and delta > 0.):
        raise ValueError("delta: a positive number")
    rho_ref = so_reference_density(box, reference)
    n = particles.n if isinstance(particles, HaloCatalogue) else np.shape(particles)[0]
    if edges is None:
        rmax = min(SO_RMAX, 0.45 * min(L)) if rmax is None else float(rmax)
        if rmin is None:
            rmin = min(0.25 * (L[0] * L[1] * L[2] / max(n, 1)) ** (1. / 3.), 0.5 * rmax)
        if not (0. < float(rmin) < rmax) or int(nbins) < 1:
            raise ValueError("0 < rmin < rmax and nbins >= 1")
        edges = np.geomspace(float(rmin), rmax, int(nbins) + 1)
    e = profile_edges(L, edges)
    sw = _CentreSweeps(box, "spherical_overdensity", centres, particles, velocities, e[-1], e.size - 1, timings)
    rows = sw.profiles(e)
    prof = HaloProfiles(e, rows[:, 0], rows[:, 1:], _profile_mass(box, sw.n, particle_mass))
    radius, mass, status = so_from_enclosed(e, prof.enclosed, prof.particle_mass, rho_ref, delta)
    count, com, vm, sigma = sw.apertures(np.where(status == 0, radius * radius, 0.))
    eng, nh = sw.eng, sw.nh
    vel = HaloCatalogue(eng, vm, nh) if sw.has_vel else None
    return SOHalos(eng, sw.cbuf, nh, radius, mass, status, count, HaloCatalogue(eng, com, nh), vel, sigma, prof, delta, rho_ref)


# ---------------------------------------------------------------------- three-point correlation multipoles
TRIPLET_MAX_NR, TRIPLET_MAX_L, TRIPLET_MAX_PROBE = 32, 10, 64       # FB_TRIP_MAX_NR, _MAX_L, _MAX_PROBE of fb_triplets.hip


def triplet_edges(L, edges, lmax=10):
    """The checked radial edges and order of ``triplet_multipoles``: strictly ascending, finite, edges[0] > 0, at most 32 bins,
    the last edge below min(L) / 2; lmax an integer from 0 to 10.  ValueError otherwise."""
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or not np.all(np.isfinite(e)) or not e[0] > 0. or not np.all(e[1:] > e[:-1]):
        raise ValueError("edges: a strictly ascending array of at least 2 finite values, edges[0] > 0")
    if e.size - 1 > TRIPLET_MAX_NR:
        raise ValueError("edges: at most %d bins, got %d" % (TRIPLET_MAX_NR, e.size - 1))
    if not e[-1] < 0.5 * min(L):
        raise ValueError("edges: the last edge %.6g Mpc must be below half the shortest box side (%.6g Mpc)" % (e[-1], 0.5 * min(L)))
    if isinstance(lmax, bool) or int(lmax) != lmax or not 0 <= int(lmax) <= TRIPLET_MAX_L:
        raise ValueError("lmax: an integer from 0 to %d" % TRIPLET_MAX_L)
    return e, int(lmax)


def triplet_fx_bits(n, wmax=1.):
    """(F_a, F_S, F_M): the fractional bits of the device's fixed-point sums of a_lm, S and M for n particles of largest
    |weight| wmax: 93 - e with bound < 2^e (frexp), the bounds being 2 n wmax, n wmax^2 and 4 (n wmax)^3."""
    def bits(bound):
        return 93 - (int(np.frexp(bound)[1]) if bound > 0. else 0)
    nw = float(n) * float(wmax)
    return bits(2. * nw), bits(float(n) * float(wmax) * float(wmax)), bits(4. * nw * nw * nw)


def triplet_device_bytes(n, cells, nr=TRIPLET_MAX_NR, lmax=TRIPLET_MAX_L, weighted=False, host_positions=False, nprobe=0):
    """Device bytes triplet_multipoles allocates beside the catalogue: the work buffer (32 bytes a particle -- the permuted
    positions, cell ids and permutation --, 8 more with weights, and the workgroups' partial sums), the outputs, and the
    uploads of host positions and weights."""
    ncells = int(cells[0]) * int(cells[1]) * int(cells[2])
    need = int(_lib.load().fb_triplet_work_bytes(int(n), ncells, int(nr), int(lmax), 1 if weighted else 0))
    need += 8 * (lmax + 1) * nr * nr + 8 * nr + 8 * nprobe * (lmax + 1) ** 2 * nr + 512
    return need + (24 * n + 32 if host_positions else 0) + (8 * n + 32 if weighted else 0)


def three_point_normalisation(edges, L, W_d):
    """(volumes, norm) of ``three_point``, pure numpy: V_b = 4 pi / 3 (e_(b+1)^3 - e_b^3) and norm(b1, b2) = W_d^3 / V^2
    V_b1 V_b2, V = Lx Ly Lz: the expected weighted triplet count of an unclustered catalogue of total weight W_d."""
    e = np.asarray(edges, dtype=np.float64)
    vol = (4. * np.pi / 3.) * (e[1:] ** 3 - e[:-1] ** 3)
    V = float(L[0]) * float(L[1]) * float(L[2])
    return vol, float(W_d) ** 3 / V ** 2 * vol[:, None] * vol[None, :]


def triplet_multipoles(box, positions, edges, lmax=10, weights=None, probe=None, timings=None):
    """The raw three-point multipole moments of a weighted catalogue in the periodic box, summed on the device (Slepian &
    Eisenstein 2015; definition and design in DESIGN.md section 4): per primary i and radial bin b the harmonic coefficients
    a_lm(b) = sum_j w_j Y_lm(u_ij) of its neighbours, then M_l(b1, b2) = sum_i w_i ((4 pi / (2 l + 1)) sum_m a_lm(b1) a_lm(b2) -
    [b1 = b2] sum_j w_j^2), which is the sum over ordered triplets (i; j != k) of w_i w_j w_k P_l(u_ij . u_ik).  ``positions``:
    a HaloCatalogue of this box or a host (n, 3) array in Mpc, periodic and wrapped on read; ``weights``: n host values of any
    sign (default 1); ``edges``: radial edges in Mpc, edges[0] > 0, lower edge inclusive, upper exclusive, decided on squares
    (``triplet_edges``); ``probe``: up to 64 indices into ``positions`` whose a_lm are returned as well; ``timings``: a dict that
    receives the milliseconds of the stages.  Returns (M float64 (lmax + 1, nr, nr), npairs int64 (nr,): the ordered pairs of
    ``pair_counts``, alm float64 (nprobe, (lmax + 1)^2, nr) -- index l^2 + l + m -- or None).  The sums are fixed-point: the same
    bit for bit from call to call and for any order of the particles.  ValueError: bad arguments, a host position or weight
    that is not finite (all before the device is touched), a device position that is not finite or too large to wrap into
    the box; MemoryError before any allocation if the work memory does not fit."""
    eng = box.engine
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    e, lmax = triplet_edges(L, edges, lmax)
    nr = e.size - 1
    n, hp, cat = _pair_positions(eng, positions, "positions")
    if n > 2 ** 31 - 2:
        raise ValueError("triplet_multipoles: at most 2^31 - 2 particles")
    if hp is not None and not np.all(np.isfinite(hp)):
        raise ValueError("positions: a position is not finite")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != n:
            raise ValueError("weights: expected %d values, got %d" % (n, w.size))
        if not np.all(np.isfinite(w)):
            raise ValueError("weights: a weight is not finite")
    pr = np.zeros(0, dtype=np.int32)
    if probe is not None:
        pq = np.asarray(probe).reshape(-1)
        if pq.size > TRIPLET_MAX_PROBE or (pq.size and (np.any(pq != np.floor(pq)) or pq.min() < 0 or pq.max() >= n)):
            raise ValueError("probe: at most %d indices into the %d positions" % (TRIPLET_MAX_PROBE, n))
        pr = np.ascontiguousarray(pq, dtype=np.int32)
    nlm = (lmax + 1) ** 2
    cells = pair_cells(L, (e[-1],) * 3, max(n, 1))
    eng.need_memory(triplet_device_bytes(n, cells, nr, lmax, w is not None, hp is not None, pr.size),
                    "triplet_multipoles: %d particles in %d x %d x %d cells take" % ((n,) + cells))
    keep = []
    pptr = wptr = None
    if n:
        if cat is not None:
            pptr = cat.ptr
        else:
            keep.append(eng.upload_raw(hp))
            pptr = keep[-1].ptr
        if w is not None:
            keep.append(eng.upload_raw(w))
            wptr = keep[-1].ptr
    wbytes = int(eng.lib.fb_triplet_work_bytes(n, cells[0] * cells[1] * cells[2], nr, lmax, 1 if w is not None else 0))
    work, mout, pout = eng._alloc_bytes(wbytes), eng._alloc_bytes(8 * (lmax + 1) * nr * nr), eng._alloc_bytes(8 * nr)
    aout = eng._alloc_bytes(8 * pr.size * nlm * nr) if pr.size else None
    e2 = np.ascontiguousarray(e * e)
    bad = ctypes.c_int32(0)
    ms = (ctypes.c_double * 3)()
    _lib.call("fb_triplet_multipoles", eng._plan, pptr, wptr, n, (ctypes.c_int32 * 3)(*cells),
              e2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nr, lmax, work.ptr, wbytes, mout.ptr, pout.ptr,
              pr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if pr.size else None, int(pr.size), aout.ptr if pr.size else None,
              ctypes.byref(bad), ms if timings is not None else None, eng.stream)
    if bad.value & 1:
        raise ValueError("triplet_multipoles: a position is not finite, or too large to wrap into the box")
    if bad.value:
        raise ValueError("triplet_multipoles: a weight is not finite, or (n max |w|)^3 overflows")
    M = eng.download_raw(mout, (lmax + 1, nr, nr))
    npairs = eng.download_raw(pout, nr, np.uint64).astype(np.int64)
    alm = eng.download_raw(aout, (pr.size, nlm, nr)) if pr.size else None
    if timings is not None:
        timings.update(bin_ms=ms[0], sweep_ms=ms[1], finish_ms=ms[2], cells=cells)
    return M, npairs, alm


class ThreePoint(object):
    """The three-point correlation multipoles of ``three_point``.  Members: ``edges`` (nr + 1, Mpc);
    ``r``, the arithmetic bin midpoints; ``volumes`` V_b = 4 pi / 3 (e_(b+1)^3 - e_b^3); ``lmax``; ``multipoles`` (lmax + 1,
    nr, nr): the raw moments M_l(b1, b2) of ``triplet_multipoles``; ``npairs`` int64 (nr,): the ordered pairs of the sweep's
    catalogue; ``zeta`` (lmax + 1, nr, nr) = (2 l + 1) M_l / norm, norm = W_d^3 / V^2 V_b1 V_b2 (``three_point_normalisation``),
    minus 1 at l = 0 without randoms; ``connected``: True with randoms (zeta is the connected zeta_l(r1, r2) of the D - R
    field), False without (the multipoles of the full three-point function, xi(r1) + xi(r2) + xi(r3) included); ``n_data``,
    ``n_random``; ``catalogue`` and ``weights``: what the sweep ran on (data then randoms, joined on the device; None
    weights: all 1)."""

    def __init__(self, edges, L, lmax, M, npairs, W_d, connected, n_data, n_random, catalogue=None, weights=None):
        self.edges = np.array(edges, dtype=np.float64)
        self.r = 0.5 * (self.edges[1:] + self.edges[:-1])
        self.lmax, self.connected, self.n_data, self.n_random = int(lmax), bool(connected), int(n_data), int(n_random)
        self.multipoles, self.npairs = np.array(M, dtype=np.float64), np.array(npairs, dtype=np.int64)
        self.catalogue, self.weights = catalogue, weights
        self.volumes, norm = three_point_normalisation(self.edges, L, W_d)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.zeta = (2. * np.arange(self.lmax + 1) + 1.)[:, None, None] * self.multipoles / norm[None, :, :]
        if not self.connected:
            self.zeta[0] -= 1.

    def __repr__(self):
        return "ThreePoint(lmax=%d, %d bins, %d data, %d randoms, %s)" % (self.lmax, self.edges.size - 1, self.n_data, self.n_random,
                                                                          "connected" if self.connected else "full")


def three_point(box, data, edges, lmax=10, randoms=None, weights=None, seed=None):
    """CosmoBox.three_point: see there."""
    from . import recon
    eng = box.engine
    L = (float(box.Lx), float(box.Ly), float(box.Lz))
    e, lmax = triplet_edges(L, edges, lmax)
    nd, hd, cd = _pair_positions(eng, data, "data")
    if hd is not None and not np.all(np.isfinite(hd)):
        raise ValueError("data: a position is not finite")
    wd = None
    if weights is not None:
        wd = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if wd.size != nd or not np.all(np.isfinite(wd)):
            raise ValueError("weights: %d finite values" % nd)
    W_d = float(np.sum(wd)) if wd is not None else float(nd)
    if randoms is None:
        M, npairs, _ = triplet_multipoles(box, data, e, lmax, weights=wd)
        return ThreePoint(e, L, lmax, M, npairs, W_d, False, nd, 0, data if cd is not None else None, wd)
    if isinstance(randoms, HaloCatalogue) or np.ndim(randoms) == 2:
        nrn, hr, cr = _pair_positions(eng, randoms, "randoms")
        if hr is not None and not np.all(np.isfinite(hr)):
            raise ValueError("randoms: a position is not finite")
    else:
        if isinstance(randoms, bool) or np.ndim(randoms) != 0 or not np.isfinite(randoms) or randoms <= 0:
            raise ValueError("randoms: None, a positive number per datum, or a catalogue")
        nrn, hr = int(round(float(randoms) * nd)), None
        if nrn > 2 ** 31 - 2 - nd:
            raise ValueError("three_point: at most 2^31 - 2 particles, data and randoms together")
        cr = recon.uniform_catalogue(box, nrn, seed=seed) if nrn else None
    if nd + nrn > 2 ** 31 - 2:
        raise ValueError("three_point: at most 2^31 - 2 particles, data and randoms together")
    if nd == 0 or nrn == 0:
        raise ValueError("three_point: randoms need at least one datum and one random point")
    cells = pair_cells(L, (e[-1],) * 3, nd + nrn)
    eng.need_memory(triplet_device_bytes(nd + nrn, cells, e.size - 1, lmax, True) + 24 * (nd + nrn),
                    "three_point: %d data and %d randoms in %d x %d x %d cells take" % ((nd, nrn) + cells))
    # data then randoms in one buffer on the device; the randoms weigh -W_d / n_r each (Szapudi & Szalay: N = D - R)
    joined = eng._alloc_bytes(24 * (nd + nrn))
    for off, m, host, cat in ((0, nd, hd, cd), (24 * nd, nrn, hr, cr)):
        if cat is not None:
            _lib.call("fb_memcpy_d2d", joined.ptr + off, cat.ptr, 24 * m, eng.stream)
        else:
            _lib.call("fb_memcpy_h2d", joined.ptr + off, host.ctypes.data_as(ctypes.c_void_p), 24 * m, eng.stream)
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    w = np.concatenate([wd if wd is not None else np.ones(nd), np.full(nrn, -W_d / nrn)])
    cat = HaloCatalogue(eng, joined, nd + nrn)
    M, npairs, _ = triplet_multipoles(box, cat, e, lmax, weights=w)
    return ThreePoint(e, L, lmax, M, npairs, W_d, True, nd, nrn, cat, w)


def paint(box, positions, weights=None, window='cic', compensated=False):
    """CosmoBox.paint_catalogue: see there."""
    eng, N = box.engine, box.N
    if window not in WINDOWS:
        raise ValueError("window must be one of %s" % sorted(WINDOWS))
    keep = []
    if isinstance(positions, HaloCatalogue):
        if positions.engine is not eng:
            raise ValueError("positions: a catalogue of this box")
        n, pptr = positions.n, positions.ptr
    else:
        p = np.ascontiguousarray(positions, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("positions: an (n, 3) array")
        n = p.shape[0]
        buf = eng.upload_raw(p) if n else None
        keep.append(buf)
        pptr = buf.ptr if n else None
    wptr = None
    if weights is not None:
        if hasattr(weights, "data_ptr"):          # a device tensor: fp64, contiguous, n values
            if str(getattr(weights, "dtype", "")) != "torch.float64" or not weights.is_contiguous() \
                    or weights.numel() != n or not weights.is_cuda:
                raise ValueError("weights: a contiguous float64 device tensor of %d values" % n)
            wptr = weights.data_ptr() if n else None
        else:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if w.size != n:
                raise ValueError("weights: expected %d values, got %d" % (n, w.size))
            if n:
                wb = eng.upload_raw(w)
                keep.append(wb)
                wptr = wb.ptr
    out = eng.empty(REAL)
    _lib.call("fb_paint", eng._plan, pptr, wptr, int(n), WINDOWS[window], out.ptr, eng.stream)
    if compensated:
        work = eng.empty("half")
        _lib.call("fb_paint_compensate", eng._plan, out.ptr, work.ptr, WINDOWS[window], eng.stream)
    eng.sync()                          # host arrays behind the uploads must outlive the copies
    return out
