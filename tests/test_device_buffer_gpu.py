"""GPU: Engine.upload_raw -> Engine.download_raw round trips, the result classes on top of them, and Engine.need_memory, on
one 16^3 single-precision box.  Every buffer is a few hundred bytes."""
import functools

import numpy as np
import pytest

from fastbox_amd import CosmoBox, default_cosmo
from fastbox_amd.halos import DeviceLabels, HaloCatalogue

pytestmark = pytest.mark.gpu
DTYPES = [np.int32, np.uint8, np.uint64, np.float64]


@functools.lru_cache(maxsize=None)
def _engine():
    return CosmoBox(cosmo=default_cosmo, box_scale=100., nsamp=16, realise_now=False, precision="f32", rng="device", seed=1).engine


def _pattern(shape, dtype, seed=0):
    """Every byte random; a float64's top byte is kept small so that none is a NaN."""
    raw = np.random.RandomState(seed).randint(0, 256, int(np.prod(shape)) * np.dtype(dtype).itemsize).astype(np.uint8)
    if np.dtype(dtype).kind == "f":
        raw[7::8] &= 0x3F
    return raw.view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1,), (7, 3), (5, 4, 3)])
def test_upload_download_round_trip(shape, dtype):
    eng = _engine()
    a = _pattern(shape, dtype)
    buf = eng.upload_raw(a)
    got = eng.download_raw(buf, shape, dtype)
    assert got.shape == shape and got.dtype == np.dtype(dtype)
    assert got.tobytes() == a.tobytes()
    assert eng.download_raw(buf.ptr, shape, dtype).tobytes() == a.tobytes()         # a raw pointer serves as well


@pytest.mark.parametrize("dtype", DTYPES)
def test_download_with_an_offset_into_a_larger_buffer(dtype):
    eng = _engine()
    item = np.dtype(dtype).itemsize
    a = _pattern((40,), dtype, seed=1)
    buf = eng.upload_raw(a)
    got = eng.download_raw(buf, (7, 3), dtype, offset=11 * item)
    assert got.tobytes() == a[11:32].tobytes()
    assert eng.download_raw(buf, 1, dtype, offset=39 * item)[0] == a[39]
    assert eng.download_raw(buf, (0, 3), dtype, offset=40 * item).shape == (0, 3)   # empty: no device call


def test_catalogue_and_labels_give_back_what_was_uploaded():
    eng = _engine()
    n = 37
    p = np.random.RandomState(2).uniform(0., 100., (n, 3))
    lab = np.random.RandomState(3).randint(-1, 9, n).astype(np.int32)
    cat, labels = HaloCatalogue(eng, eng.upload_raw(p), n), DeviceLabels(eng, eng.upload_raw(lab), n)
    assert cat.shape == (n, 3) and cat.dtype == np.float64 and len(cat) == n and cat.n == n
    assert labels.shape == (n,) and labels.dtype == np.int32 and len(labels) == n
    hp, hl = np.asarray(cat), np.asarray(labels)
    assert np.array_equal(hp, p) and hp.dtype == np.float64 and not hp.flags.writeable
    assert np.array_equal(hl, lab) and hl.dtype == np.int32 and not hl.flags.writeable
    assert np.asarray(cat) is hp and np.asarray(labels, dtype=np.int32) is hl
    assert np.array_equal(np.asarray(labels, dtype=np.int64), lab.astype(np.int64))
    empty = HaloCatalogue(eng, None, 0)
    assert empty.ptr is None and np.asarray(empty).shape == (0, 3)


def test_need_memory(monkeypatch):
    eng = _engine()
    eng.need_memory(1, "one byte takes")
    monkeypatch.setattr(eng, "free_bytes", lambda: 1 << 10)
    eng.need_memory(1 << 10, "what is free takes")
    with pytest.raises(MemoryError, match="work memory") as e:
        eng.need_memory(3 << 29, "test: %d things take" % 5)
    assert str(e.value) == "test: 5 things take 1.50 GiB of work memory, 0.00 GiB are free"
