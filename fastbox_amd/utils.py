"""
Survey geometry helpers on the host (the reference's fastbox/utils.py).
"""
import numpy as np

from .box import _ccl

LINE_FREQ = 1420.405752


def comoving_dimensions_from_survey(cosmo, angular_extent, freq_range=None, z_range=None, line_freq=1420.405752):
    """Comoving dimensions and central redshift of a survey volume from its angular extent and its frequency or redshift
    range (utils.py:8-67): returns ``zc, (Lx, Ly, Lz)`` in Mpc.

    ``angular_extent``: (deg, deg) along x and y; exactly one of ``freq_range`` (MHz) and ``z_range``; ``line_freq``: the
    rest frequency of the line in MHz.  Lz = r(zmax) - r(zmin); zc is where r reaches (r(zmin) + r(zmax)) / 2, by linear
    interpolation on 100 redshifts, as the reference does; Lx, Ly = extent (pi / 180) r_trans(zc): the small-angle box.

    Distances come from the box's cosmology provider -- pyccl where it is installed, else ``fastbox_amd.cosmology`` (flat
    LCDM, where the radial and the transverse comoving distance are the same function).  Agreement with pyccl's distances
    is not verified: pyccl was not available where this was written."""
    if (freq_range is not None and z_range is not None) or (freq_range is None and z_range is None):
        raise ValueError("Must specify either freq_range of z_range.")
    if len(angular_extent) != 2:
        raise ValueError("angular_extent must be tuple of length 2")
    if freq_range is not None:
        if len(freq_range) != 2:
            raise ValueError("freq_range must be tuple of length 2")
        z_range = (line_freq / freq_range[0] - 1., line_freq / freq_range[1] - 1.)
    if len(z_range) != 2:
        raise ValueError("z_range must be tuple of length 2")
    zmin, zmax = sorted(z_range)
    rmin = float(_ccl.comoving_radial_distance(cosmo, 1. / (1. + zmin)))
    rmax = float(_ccl.comoving_radial_distance(cosmo, 1. / (1. + zmax)))
    Lz = rmax - rmin
    _z = np.linspace(zmin, zmax, 100)
    _r = np.asarray(_ccl.comoving_radial_distance(cosmo, 1. / (1. + _z)), dtype=np.float64)
    rc = 0.5 * (rmax + rmin)
    zc = float(np.interp(rc, _r, _z))
    r_trans = float(_ccl.comoving_angular_distance(cosmo, 1. / (1. + zc)))
    Lx = angular_extent[0] * np.pi / 180. * r_trans
    Ly = angular_extent[1] * np.pi / 180. * r_trans
    return zc, (Lx, Ly, Lz)
