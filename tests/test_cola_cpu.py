"""CPU: the COLA host coefficients against Einstein-de Sitter closed forms, the numpy statement's 2LPT against analytic
fields and a 1-D Zel'dovich run, and the library's new entry points."""
import os

import numpy as np
import pytest

from fastbox_amd import cola
from fastbox_amd.cosmology import Cosmology

from . import cola_numpy as cn

EDS = Cosmology(Omega_c=0.95, Omega_b=0.05, h=0.7)
LCDM = Cosmology(Omega_c=0.25, Omega_b=0.05, h=0.7)


@pytest.mark.parametrize("a0,a1", [(1. / 16., 1.), (0.01, 0.02), (0.3, 0.31), (1. / 100., 1. / 50.)])
def test_integrals_einstein_de_sitter(a0, a1):
    g = cola.Growth(EDS)
    assert abs(g.K(a0, a1) - 2. * (np.sqrt(a1) - np.sqrt(a0))) < 1e-12
    assert abs(g.Dr(a0, a1) - 2. * (a0 ** -0.5 - a1 ** -0.5)) < 1e-12 * max(1., a0 ** -0.5)


@pytest.mark.parametrize("a", [0.01, 1. / 16., 0.5, 1.])
def test_growth_einstein_de_sitter(a):
    g = cola.Growth(EDS)
    assert abs(g.D1(a) - a) < 1e-12
    assert abs(g.P1(a) - a ** 1.5) < 1e-12
    assert abs(g.D2(a) + 3. / 7. * a * a) < 1e-12
    assert abs(g.P2(a) + 6. / 7. * a ** 2.5) < 1e-12


def test_launch_table_shape_and_telescoping():
    g = cola.Growth(LCDM)
    n = 5
    tab = cola.launch_table(g, 0., 15., n)
    assert tab.shape == (3 + 6 * (n + 1),)
    rows = tab[3:].reshape(n + 1, 6)
    a = cola.steps(0., 15., n)
    # kicks cover [a_0, a_n] exactly once, drifts [a_0, a_n]; the last launch does not drift
    assert abs(rows[:, 0].sum() - g.K(a[0], a[-1])) < 1e-12
    assert abs(rows[:, 1].sum() - (g.P1(a[-1]) - g.P1(a[0]))) < 1e-12
    assert abs(rows[:, 4].sum() - (g.D1(a[-1]) - g.D1(a[0]))) < 1e-12
    assert np.all(rows[-1, 3:] == 0.) and np.all(rows[:-1, 3] > 0.)
    assert tab[2] == 1.5 * 0.3
    assert np.array_equal(cola.launch_table(g, 0., 15., 0), [g.D1(1.), g.D2(1.), 1.5 * 0.3])


def test_library_exports_cola_entries():
    from fastbox_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library()
    lib = _lib.load()
    for name in ("fb_cola_lpt", "fb_cola_init", "fb_cola_force", "fb_cola_kick", "fb_cola_velocity",
                 "fb_cola_grid_velocity", "fb_cola_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # fb_version stays 102: tests/test_halos_cpu.py pins that value; the entries are found by their symbols
    assert lib.fb_version() >= 102


def _axes(N, L):
    x = np.arange(N) * (L / N)
    return np.meshgrid(x, x, x, indexing="ij")


def test_lpt_plane_wave():
    N, L, A, m = 32, 200., 0.05, 3
    k = 2 * np.pi * m / L
    X, Y, Z = _axes(N, L)
    psi1, psi2 = cn.lpt(A * np.cos(k * X), L)
    assert np.max(np.abs(psi1[0] + A * np.sin(k * X) / k)) < 1e-14 * L
    assert np.max(np.abs(psi1[1:])) < 1e-14 * L
    assert np.max(np.abs(psi2)) < 1e-14 * L


def test_lpt_crossed_waves():
    N, L, A, B, m = 32, 200., 0.05, 0.03, 2
    k = 2 * np.pi * m / L
    X, Y, Z = _axes(N, L)
    psi1, psi2 = cn.lpt(A * np.cos(k * X) + B * np.cos(k * Y), L)
    want = A * B / (2 * k) * np.array([np.sin(k * X) * np.cos(k * Y), np.cos(k * X) * np.sin(k * Y), 0. * X])
    assert np.max(np.abs(psi2 - want)) < 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(psi1[0] + A * np.sin(k * X) / k)) < 1e-14 * L


def test_zeldovich_plane_wave_einstein_de_sitter():
    """1-D: Zel'dovich is exact before shell crossing, so the residual momentum stays small.  The displacements are larger than
    a cell from the start (2.9 cells at z = 3, 5.7 at z = 1, no shell crossing: D1 A = 0.75): CIC painting of a lattice whose
    displacements are below a cell rectifies the density, which is a property of the mass assignment,
    not of the COLA stepping this test is about."""
    N, L, A = 48, 100., 1.5
    k = 2 * np.pi / L
    X, _, _ = _axes(N, L)
    out = cn.run(A * np.cos(k * X), L, EDS, redshift=1., redshift_init=3., n_steps=6)
    g = cola.Growth(EDS)
    P1 = g.P1(0.5)
    ratio = np.sqrt(np.mean(out["pres"][:, 0] ** 2)) / np.sqrt(np.mean((P1 * out["psi1"][:, 0]) ** 2))
    assert ratio < 0.01, ratio
    assert np.max(np.abs(out["pres"][:, 1:])) < 1e-12 * np.max(np.abs(out["pres"][:, 0]))


def test_scheme_growth():
    g = cola.Growth(LCDM)
    assert cola.scheme_growth(g, 0., 15., 0) == 1.
    assert 0.94 < cola.scheme_growth(g, 0., 15., 16) < 0.96          # the default: long first steps lose growth
    assert abs(cola.scheme_growth(g, 0., 15., 256) - 1.) < 1e-3
    assert abs(cola.scheme_growth(g, 49., 99., 100) - 1.) < 1e-5
