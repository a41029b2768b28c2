"""IJ objects initialised with HYPRE_MEMORY_DEVICE on a machine without a HIP device: every call that would read a device pointer is
refused with the "no HIP device" error and dereferences nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMM, DEVICE = 0x44000000, 1


@pytest.fixture(scope="module")
def L():
    import hypredrive_amd as h
    if h.device_count() > 0:
        pytest.skip("a GPU is present: host pointers must not reach the device path")
    L = h.load()
    vp = C.c_void_p
    L.HYPRE_IJMatrixCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.HYPRE_IJVectorCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.HYPRE_IJMatrixInitialize_v2.argtypes = L.HYPRE_IJVectorInitialize_v2.argtypes = [vp, C.c_int]
    L.HYPRE_IJMatrixSetValues.argtypes = L.HYPRE_IJMatrixAddToValues.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.HYPRE_IJVectorSetValues.argtypes = L.HYPRE_IJVectorAddToValues.argtypes = L.HYPRE_IJVectorGetValues.argtypes = [vp, C.c_int, vp, vp]
    L.HYPRE_IJMatrixDestroy.argtypes = L.HYPRE_IJVectorDestroy.argtypes = [vp]
    L.HYPRE_DescribeError.argtypes = [C.c_int, C.c_char_p]
    return L


def _text(L):
    buf = C.create_string_buffer(128)
    L.HYPRE_DescribeError(L.HYPRE_GetError(), buf)
    L.HYPRE_ClearAllErrors()
    return buf.value.decode()


def test_device_matrix_calls_are_refused_without_a_device(L):
    m = C.c_void_p()
    assert L.HYPRE_IJMatrixCreate(COMM, 0, 3, 0, 3, C.byref(m)) == 0
    assert L.HYPRE_IJMatrixInitialize_v2(m, DEVICE) == 0
    ncols, rows = np.ones(4, dtype=np.int32), np.arange(4, dtype=np.int64)
    cols, vals = np.arange(4, dtype=np.int64), np.ones(4)
    for fn in (L.HYPRE_IJMatrixSetValues, L.HYPRE_IJMatrixAddToValues):
        L.HYPRE_ClearAllErrors()
        assert fn(m, 4, ncols.ctypes.data, rows.ctypes.data, cols.ctypes.data, vals.ctypes.data) != 0
        assert "no HIP device" in _text(L)
    L.HYPRE_IJMatrixDestroy(m)


def test_device_vector_calls_are_refused_without_a_device(L):
    v = C.c_void_p()
    assert L.HYPRE_IJVectorCreate(COMM, 0, 3, C.byref(v)) == 0
    assert L.HYPRE_IJVectorInitialize_v2(v, DEVICE) == 0
    idx, val = np.arange(4, dtype=np.int64), np.ones(4)
    for fn, ix in ((L.HYPRE_IJVectorSetValues, idx.ctypes.data), (L.HYPRE_IJVectorAddToValues, None), (L.HYPRE_IJVectorGetValues, idx.ctypes.data)):
        L.HYPRE_ClearAllErrors()
        assert fn(v, 4, ix, val.ctypes.data) != 0
        assert "no HIP device" in _text(L)
    assert val.tolist() == [1.0] * 4
    L.HYPRE_IJVectorDestroy(v)


def test_vector_device_pointer_is_exported_and_declared():
    import hypredrive_amd as h
    assert hasattr(h.load(), "HYPREDRV_AMD_IJVectorDevicePointer")
    txt = open(os.path.join(ROOT, "include", "HYPREDRV.h")).read()
    assert re.search(r"HYPREDRV_AMD_IJVectorDevicePointer\s*\(\s*HYPRE_IJVector\s+\w+,\s*const\s+double\s*\*\*\s*\w+,\s*HYPRE_Int\s*\*\s*\w+\)", txt)
