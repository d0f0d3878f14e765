"""TEST INFRASTRUCTURE ONLY -- numpy/ctypes binding of oracle/_ref/libvktref.so: the volkit
REFERENCE's own serial CPU code, compiled by oracle/ref/Makefile from a reference checkout
together with oracle/ref/ref_driver.cpp.  Same call shapes as oracle/binding.py, so the oracle
and the HIP kernels can be held against the reference itself.

The library is a build product (git ignores oracle/_ref/): `available()` says whether it is
there; importing this module never builds anything and never reads a reference checkout.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from oracle.binding import BPV, CODE_DTYPE, OPS, Aggregates, UNARY, Volume, _Vol, _i3

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libvktref.so")

_lib = None


def available() -> bool:
    return os.path.exists(LIB_PATH)


def _load():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError(f"{LIB_PATH} not found: build it with `make -C oracle/ref REF=<reference checkout>`")
        lib = C.CDLL(LIB_PATH)
        vp = C.POINTER(_Vol)
        lib.vkr_map.argtypes = [C.POINTER(C.c_uint8), C.c_float, C.c_int32, C.c_float, C.c_float]
        lib.vkr_unmap.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int32, C.c_float, C.c_float]
        lib.vkr_map_n.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_float, C.c_float]
        lib.vkr_unmap_n.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_float, C.c_float]
        lib.vkr_fill_range.argtypes = [vp, _i3, _i3, C.c_float]
        lib.vkr_copy_range.argtypes = [vp, vp, _i3, _i3, _i3]
        lib.vkr_arith_range.argtypes = [C.c_int32, vp, vp, vp, _i3, _i3, _i3]
        lib.vkr_resample.argtypes = [vp, vp, C.c_int32]
        lib.vkr_aggregates_range.argtypes = [vp, _i3, _i3, C.POINTER(Aggregates)]
        lib.vkr_histogram_range.argtypes = [vp, _i3, _i3, C.POINTER(C.c_uint64), C.c_uint64]
        lib.vkr_transform_range1.argtypes = [vp, _i3, _i3, UNARY]
        _lib = lib
    return _lib


def _ok(err, what):
    if err != 0:
        raise RuntimeError(f"reference {what} returned error {err}")


def map_voxel(value: float, fmt: int, lo: float = 0.0, hi: float = 1.0) -> bytes:
    buf = (C.c_uint8 * 8)()
    _load().vkr_map(buf, value, fmt, lo, hi)
    return bytes(buf[: BPV.get(fmt, 0)])


def unmap_voxel(data: bytes, fmt: int, lo: float = 0.0, hi: float = 1.0) -> float:
    buf = (C.c_uint8 * 8)(*bytes(data)[:8])
    v = C.c_float(0.0)
    _load().vkr_unmap(C.byref(v), buf, fmt, lo, hi)
    return v.value


def map_array(values, fmt: int, lo: float = 0.0, hi: float = 1.0, init=0) -> np.ndarray:
    vals = np.ascontiguousarray(values, dtype=np.float32)
    codes = np.full(vals.shape, init, dtype=CODE_DTYPE[fmt])
    _load().vkr_map_n(codes.ctypes.data, vals.ctypes.data, vals.size, BPV[fmt], fmt, lo, hi)
    return codes


def unmap_array(codes, fmt: int, lo: float = 0.0, hi: float = 1.0, init=0.0) -> np.ndarray:
    c = np.ascontiguousarray(codes, dtype=CODE_DTYPE[fmt])
    vals = np.full(c.shape, init, dtype=np.float32)
    _load().vkr_unmap_n(vals.ctypes.data, c.ctypes.data, c.size, BPV[fmt], fmt, lo, hi)
    return vals


def fill_range(v: Volume, first, last, value: float) -> None:
    _load().vkr_fill_range(v.ref, _i3(*first), _i3(*last), value)


def copy_range(dst: Volume, src: Volume, first, last, off=(0, 0, 0)) -> None:
    _ok(_load().vkr_copy_range(dst.ref, src.ref, _i3(*first), _i3(*last), _i3(*off)), "CopyRange")


def arith_range(op, dst: Volume, s1: Volume, s2: Volume, first, last, off=(0, 0, 0)) -> None:
    code = OPS.index(op) if isinstance(op, str) else int(op)
    _ok(_load().vkr_arith_range(code, dst.ref, s1.ref, s2.ref, _i3(*first), _i3(*last), _i3(*off)), OPS[code] + "Range")


def resample(dst: Volume, src: Volume, filter_mode: int) -> None:
    _load().vkr_resample(dst.ref, src.ref, filter_mode)


def transform_range1(v: Volume, first, last, fn) -> None:
    cb = UNARY(lambda x, y, z, b, f, lo, hi: fn(x, y, z, b, f, lo, hi))
    _ok(_load().vkr_transform_range1(v.ref, _i3(*first), _i3(*last), cb), "TransformRange")


def aggregates_range(v: Volume, first, last) -> Aggregates:
    out = Aggregates()
    _ok(_load().vkr_aggregates_range(v.ref, _i3(*first), _i3(*last), C.byref(out)), "ComputeAggregatesRange")
    return out


def histogram_range(v: Volume, first, last, num_bins: int) -> np.ndarray:
    """Bin counts as a uint64 array.  The reference indexes its bins unchecked: the caller must
    have made sure that every voxel's bin lies in [0, num_bins)."""
    bins = np.zeros(num_bins, dtype=np.uint64)
    _ok(_load().vkr_histogram_range(v.ref, _i3(*first), _i3(*last), bins.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    num_bins), "ComputeHistogramRange")
    return bins
