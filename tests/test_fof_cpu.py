"""CPU: the library cross-compiles with the friends-of-friends source and exports its entries, the ctypes prototypes list
them, the version is unchanged, and find_halos_fof refuses bad arguments before it touches a device."""
import os
import types

import numpy as np
import pytest

FOF = ("fb_fof_work_bytes", "fb_fof_link", "fb_fof_sizes", "fb_fof_catalogue")


def _lib():
    from fastbox_amd import _lib
    _lib.build_library()                # the incremental make: a library older than its sources is rebuilt, not trusted
    return _lib, _lib.load()


def test_library_exports_fof_entries():
    _l, lib = _lib()
    for name in FOF:
        assert hasattr(lib, name) and name in _l.SIGNATURES, name
    assert lib.fb_version() == 102
    src = open(os.path.join(_l.CSRC, "Makefile")).read()
    assert "fb_fof.hip" in src


def test_work_bytes_cover_the_buffers():
    _l, lib = _lib()
    n, ncells = 1000, 64
    # permuted positions, cell ids, permutation, the cell table twice, the overflow tiles
    floor = 24 * n + 4 * n + 4 * n + 4 * (2 * ncells + 1) + 8 * (n // 64)
    got = lib.fb_fof_work_bytes(n, ncells)
    assert floor <= got <= floor + 4096
    assert lib.fb_fof_work_bytes(-1, 1) == -1 and lib.fb_fof_work_bytes(1, 0) == -1
    assert lib.fb_fof_work_bytes(0, 1) > 0


def test_arguments_are_checked_before_the_device():
    from fastbox_amd import halos
    box = types.SimpleNamespace(engine=None, Lx=8., Ly=8., Lz=8.)
    pos = np.zeros((12, 3))
    with pytest.raises(ValueError, match="linking length"):
        halos.find_halos_fof(box, pos, linking_length=4.0, absolute=True)
    with pytest.raises(ValueError, match="linking length"):
        halos.find_halos_fof(box, pos, linking_length=0.)
    with pytest.raises(ValueError, match="nmin"):
        halos.find_halos_fof(box, pos, nmin=0)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        halos.find_halos_fof(box, np.zeros((12, 2)))
    with pytest.raises(ValueError, match="velocities"):
        halos.find_halos_fof(box, pos, velocities=np.zeros((11, 3)))


def test_cells_are_no_smaller_than_the_linking_length():
    from fastbox_amd import halos
    for L, ell, n in (((64., 96., 128.), 0.7, 7000), ((1000.,) * 3, 0.2 * 1000. / 256, 256 ** 3), ((8.,) * 3, 3.9, 12),
                      ((64.,) * 3, 1.0, 40), ((8.,) * 3, 3.9999999999, 5)):
        cells = halos.fof_cells(L, ell, n)
        assert all(c >= 1 and La / c >= ell * (1. + 0.9e-9) for c, La in zip(cells, L))
        assert max(cells) <= max(4, int(round((0.5 * n) ** (1. / 3.))) + 1)
