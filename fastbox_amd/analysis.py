"""
Small data-analysis helpers on the device (the reference's fastbox/analysis.py).
"""
from . import _lib
from .device import REAL
from .filters import _as_cube


def replace_nan_with_channel_mean(field, box=None):
    """Replace every NaN of the cube by the mean of its frequency channel (last axis) over the voxels that are not NaN.
    Other voxels are copied bit for bit; a channel that is NaN throughout stays NaN.  Returns a new REAL DeviceArray."""
    cube = _as_cube(field, box)
    eng = cube.engine
    out = eng.empty(REAL)
    _lib.call("fb_replace_nan_channel_mean", eng._plan, cube.ptr, out.ptr, None, eng.stream)
    return out
