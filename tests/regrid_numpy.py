"""Numpy statements of fastbox_amd.analysis.interpolate_onto_grid and grid_catalogue (the definitions in include/fastbox_hip.h at
fb_regrid_trilinear and fb_grid_catalogue): per-axis searchsorted and an eight-corner sum; per-axis searchsorted on the linspace
edges and np.add.at.  Neither calls scipy.interpolate or np.histogramdd: tests/test_regrid_cases_cpu.py holds them to those."""
import itertools

import numpy as np


def fill_nan_channel_mean(field):
    """NaN -> the mean of the channel (last axis) over the voxels that are not NaN; an all-NaN channel stays NaN."""
    f = np.array(field, dtype=np.float64)
    flat = f.reshape(-1, f.shape[-1])
    for j in range(flat.shape[1]):
        bad = np.isnan(flat[:, j])
        if bad.any():
            flat[bad, j] = np.mean(flat[~bad, j]) if (~bad).any() else np.nan
    return f


def locate(g, p):
    """(cell, fraction, inside) of the new coordinates p on the ascending grid g."""
    g, p = np.asarray(g, dtype=np.float64), np.asarray(p, dtype=np.float64)
    i = np.clip(np.searchsorted(g, p, side='right') - 1, 0, g.size - 2)
    t = (p - g[i]) / (g[i + 1] - g[i])
    return i, t, (p >= g[0]) & (p <= g[-1])


def interpolate_onto_grid(field, coords_orig, coords_new, indexing='xy'):
    """The trilinear regrid: value = sum over the eight corners (x outermost, z innermost) of v ((wx wy) wz), zero weights
    included; NaN outside.  'xy': shape (len(y_new), len(x_new), len(z_new)), element [j, i, k] at (x_new[i], y_new[j],
    z_new[k]); 'ij': (len(x_new), len(y_new), len(z_new))."""
    f = fill_nan_channel_mean(field)
    loc = [locate(g, p) for g, p in zip(coords_orig, coords_new)]
    (ix, tx, okx), (iy, ty, oky), (iz, tz, okz) = loc
    I, J, K = ix[:, None, None], iy[None, :, None], iz[None, None, :]
    w = [(1. - tx, tx), (1. - ty, ty), (1. - tz, tz)]
    value = np.zeros((ix.size, iy.size, iz.size))
    with np.errstate(invalid='ignore'):
        for a, b, c in itertools.product((0, 1), repeat=3):
            weight = (w[0][a][:, None, None] * w[1][b][None, :, None]) * w[2][c][None, None, :]
            value = value + f[I + a, J + b, K + c] * weight
    value[~(okx[:, None, None] & oky[None, :, None] & okz[None, None, :])] = np.nan
    return value.transpose(1, 0, 2).copy() if indexing == 'xy' else value


def hist_limits(lo, hi):
    lo, hi = float(lo), float(hi)
    return (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)


def hist_bins(p, lo, hi, n):
    """Bin of every p among np.linspace(lo, hi, n + 1), -1 where p is outside [lo, hi] or NaN: searchsorted 'right' - 1, the
    last edge in the last bin."""
    p = np.asarray(p, dtype=np.float64)
    e = np.linspace(lo, hi, n + 1)
    b = np.searchsorted(e, p, side='right') - 1
    b[p == e[-1]] = n - 1
    with np.errstate(invalid='ignore'):
        b[~((p >= e[0]) & (p <= e[-1]))] = -1
    return b


def grid_catalogue(pos, w, limits, nbin):
    """(grid, (xgrid, ygrid, zgrid)): pos (n, 3); limits three (lo, hi) or None (the data's range); nbin (nx, ny, nz)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    lims = [hist_limits(*((pos[:, a].min(), pos[:, a].max()) if limits[a] is None else limits[a])) for a in range(3)]
    b = [hist_bins(pos[:, a], lims[a][0], lims[a][1], nbin[a]) for a in range(3)]
    keep = (b[0] >= 0) & (b[1] >= 0) & (b[2] >= 0)
    grid = np.zeros(tuple(nbin))
    wk = np.ones(pos.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    np.add.at(grid, (b[0][keep], b[1][keep], b[2][keep]), wk[keep])
    return grid, tuple(np.linspace(lims[a][0], lims[a][1], nbin[a]) for a in range(3))
