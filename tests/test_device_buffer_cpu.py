"""Engine.download_raw, Engine.need_memory and DeviceBuffer without a GPU or the library: a stand-in engine, and
``_lib.call`` patched so that fb_memcpy_d2h copies from a host array standing in for device memory."""
import ctypes

import numpy as np
import pytest

from fastbox_amd import _lib
from fastbox_amd.device import DeviceBuffer, Engine
from fastbox_amd.halos import ColaParticles, DeviceLabels, FoFHalos, HaloCatalogue, SOHalos
from fastbox_amd.interferometer import DeviceCounts
from fastbox_amd.recon import DeviceValues
from fastbox_amd.voids import VoidLabels
from fastbox_amd.web import ClassCube

DTYPES = [np.int32, np.uint8, np.uint64, np.float64]
SHAPES = [(5,), (7, 3), (4, 4, 4)]
GIB = 2 ** 30


class FakeEngine(object):
    """What DeviceBuffer and the two Engine methods touch: a stream, N, and the methods themselves."""
    stream = None
    N = 4
    download_raw = Engine.download_raw
    need_memory = Engine.need_memory

    def __init__(self, free=0):
        self._free = free

    def free_bytes(self):
        return self._free


class FakeMemory(object):
    """A host array in the role of a device allocation: ``ptr`` is its address."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)
        self.ptr = self.a.ctypes.data


@pytest.fixture
def copies(monkeypatch):
    """The (name, nbytes) of every _lib.call; fb_memcpy_d2h is carried out on the host, anything else is an error."""
    seen = []

    def call(name, *args):
        assert name == "fb_memcpy_d2h", name
        dst, src, nbytes, stream = args
        assert stream is None
        seen.append((name, nbytes))
        ctypes.memmove(dst, src, nbytes)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def _pattern(shape, dtype, seed=0):
    n = int(np.prod(shape))
    raw = np.random.RandomState(seed).randint(0, 256, n * np.dtype(dtype).itemsize).astype(np.uint8)
    if np.dtype(dtype).kind == "f":
        raw[7::8] &= 0x3F                      # keep the exponent away from NaN: array_equal compares values
    return raw.view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_download_raw_is_bit_exact(copies, shape, dtype):
    src = _pattern(shape, dtype)
    mem = FakeMemory(src)
    for handle in (mem, mem.ptr):                                     # anything with .ptr, or the raw pointer
        got = Engine.download_raw(FakeEngine(), handle, shape, dtype)
        assert got.shape == shape and got.dtype == np.dtype(dtype) and got.flags.writeable
        assert got.tobytes() == src.tobytes()
    assert copies == [("fb_memcpy_d2h", src.nbytes)] * 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_download_raw_offset_selects_the_bytes(copies, shape, dtype):
    item = np.dtype(dtype).itemsize
    lead = 3                                                          # elements in front of the window
    big = _pattern((lead + int(np.prod(shape)) + 2,), dtype, seed=1)
    got = Engine.download_raw(FakeEngine(), FakeMemory(big), shape, dtype, offset=lead * item)
    assert got.tobytes() == big[lead:lead + got.size].tobytes()
    assert copies == [("fb_memcpy_d2h", got.nbytes)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_download_raw_of_an_empty_shape_makes_no_call(copies, dtype):
    got = Engine.download_raw(FakeEngine(), None, (0, 3), dtype)
    assert got.shape == (0, 3) and got.dtype == np.dtype(dtype)
    assert copies == []


def test_download_raw_defaults_to_float64_and_takes_an_int_shape(copies):
    src = _pattern((6,), np.float64)
    got = Engine.download_raw(FakeEngine(), FakeMemory(src), 6)
    assert got.dtype == np.float64 and np.array_equal(got, src)


# ---- DeviceBuffer ----------------------------------------------------------------------------------------------------------
def test_device_buffer_reads_back_once_and_read_only(copies):
    src = _pattern((7, 3), np.int32)
    b = DeviceBuffer(FakeEngine(), FakeMemory(src), (7, 3), np.int32)
    assert (b.shape, b.dtype, b.ndim, b.size, len(b)) == ((7, 3), np.dtype(np.int32), 2, 21, 7)
    assert b.ptr == b._buf.ptr
    assert copies == []                                                # nothing until numpy touches it
    first = np.asarray(b)
    for _ in range(3):
        assert np.asarray(b) is first
    assert b.host() is first
    assert copies == [("fb_memcpy_d2h", src.nbytes)]
    assert np.array_equal(first, src) and not first.flags.writeable
    with pytest.raises(ValueError):
        first[0, 0] = 1


def test_device_buffer_dtype_argument(copies):
    src = _pattern((5,), np.int32)
    b = DeviceBuffer(FakeEngine(), FakeMemory(src), (5,), np.int32)
    assert np.asarray(b, dtype=b.dtype) is b.host()
    assert np.asarray(b, dtype=np.int32) is b.host()
    conv = np.asarray(b, dtype=np.float64)
    assert conv is not b.host() and conv.dtype == np.float64 and conv.flags.writeable
    assert np.array_equal(conv, src.astype(np.float64))
    assert len(copies) == 1


@pytest.mark.parametrize("make,shape,dtype", [
    (lambda e: DeviceBuffer(e, None, (0, 3), np.float64), (0, 3), np.float64),
    (lambda e: HaloCatalogue(e, None, 0), (0, 3), np.float64),
    (lambda e: DeviceLabels(e, None, 0), (0,), np.int32),
    (lambda e: DeviceValues(e, None, (0, 2)), (0, 2), np.float64),
])
def test_no_buffer_gives_an_empty_array_without_a_call(copies, make, shape, dtype):
    b = make(FakeEngine())
    assert b.ptr is None and len(b) == 0 and b.size == 0
    h = np.asarray(b)
    assert h.shape == shape and h.dtype == np.dtype(dtype) and not h.flags.writeable
    assert copies == []


# ---- the six result classes -----------------------------------------------------------------------------------------------------
def _six(eng):
    N = eng.N
    mem = lambda shape, dtype: FakeMemory(_pattern(shape, dtype, seed=2))
    return [
        (HaloCatalogue(eng, mem((5, 3), np.float64), 5), (5, 3), np.float64),
        (DeviceLabels(eng, mem((5,), np.int32), 5), (5,), np.int32),
        (VoidLabels(eng, mem((N,) * 3, np.int32), 9), (N,) * 3, np.int32),
        (DeviceValues(eng, mem((6, 2), np.float64), (6, 2)), (6, 2), np.float64),
        (ClassCube(eng, mem((N,) * 3, np.uint8)), (N,) * 3, np.uint8),
        (DeviceCounts(eng, mem((N,) * 3, np.int32)), (N,) * 3, np.int32),
    ]


def test_the_six_classes_are_device_buffers(copies):
    for obj, shape, dtype in _six(FakeEngine()):
        name = type(obj).__name__
        assert isinstance(obj, DeviceBuffer), name
        assert obj.shape == shape and obj.dtype == np.dtype(dtype), name
        assert obj.ndim == len(shape) and obj.size == int(np.prod(shape)) and len(obj) == shape[0], name
        h = np.asarray(obj)
        assert h.tobytes() == obj._buf.a.tobytes() and h.shape == shape and h.dtype == np.dtype(dtype), name
        assert np.asarray(obj, dtype=dtype) is h and not h.flags.writeable, name
    assert len(copies) == 6


def test_subclasses_keep_their_parents_attributes_and_reprs():
    eng = FakeEngine()
    for cls in (FoFHalos, ColaParticles, SOHalos):
        assert issubclass(cls, HaloCatalogue) and issubclass(cls, DeviceBuffer)
    cola = ColaParticles(eng, None, 0, None)
    assert isinstance(cola, HaloCatalogue) and isinstance(cola.velocities, HaloCatalogue) and cola.n == 0
    assert repr(cola) == "ColaParticles(0 particles)"
    fof = FoFHalos(eng, None, 0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), None, DeviceLabels(eng, None, 0), 3,
                   0.5, 2.)
    assert isinstance(fof, HaloCatalogue) and fof.n == 0 and fof.labels.n == 0 and fof.n_groups_all == 3
    assert repr(fof) == "FoFHalos(0 halos of 3 groups, linking length 0.5 Mpc)"
    assert repr(HaloCatalogue(eng, None, 0)) == "HaloCatalogue(0 halos)"
    assert repr(VoidLabels(eng, None, 9)) == "VoidLabels(9 regions, N=4)" and VoidLabels(eng, None, 9).n_labels == 9
    assert repr(DeviceValues(eng, None, (6, 2))) == "DeviceValues(shape=(6, 2))"
    assert repr(ClassCube(eng, None)) == "ClassCube(shape=(4, 4, 4))"


# ---- need_memory ------------------------------------------------------------------------------------------------------------------
def test_need_memory_passes_when_it_fits():
    FakeEngine(free=GIB).need_memory(GIB, "anything takes")
    FakeEngine(free=1).need_memory(0, "anything takes")


@pytest.mark.parametrize("what,message", [
    # the literals of the three helpers this method replaced (web._check_memory, losfit._need_memory,
    # Interferometer._need_memory), formed as they formed them for need = 1.5 GiB, free = 0.25 GiB
    ("tidal_tensor: a %d^3 grid takes" % 64, "tidal_tensor: a 64^3 grid takes 1.50 GiB of work memory, 0.25 GiB are free"),
    ("run_fit:", "run_fit: 1.50 GiB of work memory, 0.25 GiB are free"),
    ("psf: a %d^3 box takes" % 64, "psf: a 64^3 box takes 1.50 GiB of work memory, 0.25 GiB are free"),
    ("find_halos_fof: %d particles in %d x %d x %d cells take" % (1000, 4, 5, 6),
     "find_halos_fof: 1000 particles in 4 x 5 x 6 cells take 1.50 GiB of work memory, 0.25 GiB are free"),
])
def test_need_memory_message(what, message):
    with pytest.raises(MemoryError) as e:
        FakeEngine(free=GIB // 4).need_memory(3 * GIB // 2, what)
    assert str(e.value) == message


def test_need_memory_message_equals_the_former_helpers_format():
    need, have, N = 3 * GIB // 2 + 12345, GIB // 4 + 999, 48
    for what, old in (
            ("classify: a %d^3 grid takes" % N,
             "%s: a %d^3 grid takes %.2f GiB of work memory, %.2f GiB are free" % ("classify", N, need / 2. ** 30, have / 2. ** 30)),
            ("gpr_filter:", "%s: %.2f GiB of work memory, %.2f GiB are free" % ("gpr_filter", need / 2. ** 30, have / 2. ** 30)),
            ("observe: a %d^3 box takes" % N,
             "%s: a %d^3 box takes %.2f GiB of work memory, %.2f GiB are free" % ("observe", N, need / 2. ** 30, have / 2. ** 30))):
        with pytest.raises(MemoryError) as e:
            FakeEngine(free=have).need_memory(need, what)
        assert str(e.value) == old
