"""ctypes view of the reference-facing boundary (include/HYPREDRV.h): the same calls, in the
same order, that a C driver written against hypredrive makes."""
import ctypes as C

import numpy as np

from ._lib import load, LibraryError

_configured = False

# error bits (reference include/internal/error.h:16-48)
ERROR_INVALID_SOLVER = 0x00020000
ERROR_INVALID_PRECON = 0x00040000
ERROR_FILE_NOT_FOUND = 0x00080000
ERROR_FILE_UNEXPECTED_ENTRY = 0x00100000
ERROR_UNKNOWN_HYPREDRV_OBJ = 0x00200000
ERROR_NOT_INITIALIZED = 0x00400000
ERROR_UNKNOWN_TIMING = 0x00800000
ERROR_HYPRE_INTERNAL = 0x01000000
ERROR_UNSUPPORTED_AMD = 0x02000000
ERROR_MISSING_PRECON = 0x00008000
ERROR_MISSING_DOFMAP = 0x00010000
ERROR_MISSING_KEY = 0x00001000
ERROR_INVALID_KEY = 0x00000100
ERROR_INVALID_VAL = 0x00000200
ERROR_UNKNOWN = 0x80000000
MPI_COMM_WORLD = 0x44000000

# staged-transport callbacks (include/HYPREDRV.h): return 0 on success, non-zero makes the library raise on this rank
ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int)
ALLTOALLV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_long), C.c_void_p, C.POINTER(C.c_long))


def lib():
    global _configured
    L = load()
    if _configured:
        return L
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    u32 = C.c_uint32
    sig = {
        "HYPREDRV_Initialize": [], "HYPREDRV_Finalize": [],
        "HYPREDRV_Create": [C.c_int, C.POINTER(vp)], "HYPREDRV_Destroy": [C.POINTER(vp)],
        "HYPREDRV_SetLibraryMode": [vp], "HYPREDRV_InputArgsParse": [C.c_int, C.POINTER(C.c_char_p), vp],
        "HYPREDRV_InputArgsSetPreconPreset": [vp, C.c_char_p], "HYPREDRV_InputArgsSetSolverPreset": [vp, C.c_char_p],
        "HYPREDRV_InputArgsGetNumRepetitions": [vp, ip], "HYPREDRV_InputArgsGetNumLinearSystems": [vp, ip],
        "HYPREDRV_InputArgsGetNumPreconVariants": [vp, ip], "HYPREDRV_InputArgsSetPreconVariant": [vp, C.c_int],
        "HYPREDRV_LinearSystemBuild": [vp],
        "HYPREDRV_LinearSystemSetMatrixFromCSR": [vp, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong),
                                                  C.POINTER(C.c_longlong), dp],
        "HYPREDRV_LinearSystemSetRHSFromArray": [vp, C.c_longlong, C.c_longlong, dp],
        "HYPREDRV_LinearSystemSetInitialGuess": [vp, vp], "HYPREDRV_LinearSystemSetPrecMatrix": [vp, vp],
        "HYPREDRV_LinearSystemResetInitialGuess": [vp],
        "HYPREDRV_LinearSystemGetSolutionValues": [vp, C.POINTER(dp)],
        "HYPREDRV_LinearSystemGetSolutionLength": [vp, C.POINTER(C.c_longlong)],
        "HYPREDRV_LinearSystemGetSolutionNorm": [vp, C.c_char_p, dp],
        "HYPREDRV_PreconCreate": [vp], "HYPREDRV_LinearSolverCreate": [vp], "HYPREDRV_PreconSetup": [vp],
        "HYPREDRV_LinearSolverSetup": [vp], "HYPREDRV_LinearSolverApply": [vp], "HYPREDRV_PreconDestroy": [vp],
        "HYPREDRV_LinearSolverDestroy": [vp], "HYPREDRV_StatsPrint": [vp],
        "HYPREDRV_AnnotateBegin": [vp, C.c_char_p, C.c_int], "HYPREDRV_AnnotateEnd": [vp, C.c_char_p, C.c_int],
        "HYPREDRV_LinearSolverGetNumIter": [vp, ip], "HYPREDRV_LinearSolverGetConverged": [vp, ip],
        "HYPREDRV_LinearSolverGetFinalRelativeResidualNorm": [vp, dp],
        "HYPREDRV_LinearSolverGetSetupTime": [vp, dp], "HYPREDRV_LinearSolverGetSolveTime": [vp, dp],
        "HYPREDRV_AMD_CommGetUniqueId": [vp], "HYPREDRV_AMD_CommInit": [C.c_int, C.c_int, C.c_int, vp],
        "HYPREDRV_AMD_CommInitCallbacks": [C.c_int, C.c_int, C.c_int, ALLREDUCE_CB, ALLTOALLV_CB],
        "HYPREDRV_AMD_CommFinalize": [],
        "HYPREDRV_AMD_LinearSystemSetLaplacian7pt": [vp, ip, ip, dp],
        "HYPREDRV_AMD_LinearSystemSetEmptyBlock": [vp, C.c_longlong],
        "HYPREDRV_LinearSystemSetMatrix": [vp, vp], "HYPREDRV_LinearSystemSetRHS": [vp, vp],
        "HYPREDRV_LinearSystemSetDiscreteGradient": [vp, vp], "HYPREDRV_LinearSystemSetDiscreteCurl": [vp, vp],
        "HYPREDRV_LinearSystemSetCoordinates": [vp, vp, vp, vp],
        "HYPREDRV_LinearSystemSetDofmap": [vp, C.c_int, ip],
        "HYPREDRV_LinearSystemSetInterleavedDofmap": [vp, C.c_int, C.c_int],
        "HYPREDRV_LinearSystemSetContiguousDofmap": [vp, C.c_int, C.c_int],
        "HYPREDRV_LinearSystemSetNullSpace": [vp, C.c_int, C.c_int, dp],
        "HYPREDRV_LinearSystemReadMatrix": [vp],
        "HYPREDRV_AnnotateLevelBegin": [vp, C.c_int, C.c_char_p, C.c_int],
        "HYPREDRV_AnnotateLevelEnd": [vp, C.c_int, C.c_char_p, C.c_int],
        "HYPREDRV_StatsLevelGetCount": [vp, C.c_int, ip],
        "HYPREDRV_StatsLevelGetEntry": [vp, C.c_int, C.c_int, ip, ip, ip, dp, dp],
        "HYPREDRV_StatsLevelPrint": [vp, C.c_int],
        "HYPREDRV_AMD_SolvePhaseBytes": [vp, dp, dp],
        "HYPREDRV_AMD_LastResidualNorms": [vp, dp, dp, ip],
        "HYPREDRV_AMD_ProbeDominant": [vp, C.c_int, ip, dp, dp, ip],
        "HYPREDRV_AMD_LinearSolverApplyMulti": [vp, C.c_int, C.c_int, vp, vp, C.c_longlong, ip, dp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = u32
    L.HYPREDRV_ErrorCodeDescribe.argtypes = [u32]
    L.HYPREDRV_ErrorCodeDescribe.restype = None
    L.HYPREDRV_ErrorCodeClear.restype = None
    L.HYPREDRV_AMD_LastErrorMessage.restype = C.c_char_p
    _configured = True
    return L


def ij_matrix(m, ilower=0, jlower=0):
    """A scipy matrix as an assembled HYPRE_IJMatrix (a handle, c_void_p) whose rows start at ilower and whose columns start at jlower:
    the column range of a rectangular matrix is its own."""
    L = lib()
    m = m.tocsr()
    ll = C.POINTER(C.c_longlong)
    L.HYPRE_IJMatrixCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_void_p)]
    L.HYPRE_IJMatrixSetObjectType.argtypes = [C.c_void_p, C.c_int]
    L.HYPRE_IJMatrixInitialize.argtypes = L.HYPRE_IJMatrixAssemble.argtypes = L.HYPRE_IJMatrixDestroy.argtypes = [C.c_void_p]
    L.HYPRE_IJMatrixSetValues.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), ll, ll, C.POINTER(C.c_double)]
    h = C.c_void_p()
    n, nc = m.shape
    ok = L.HYPRE_IJMatrixCreate(MPI_COMM_WORLD, ilower, ilower + n - 1, jlower, jlower + nc - 1, C.byref(h)) == 0
    ok = ok and L.HYPRE_IJMatrixSetObjectType(h, 5555) == 0 and L.HYPRE_IJMatrixInitialize(h) == 0
    sizes = np.ascontiguousarray(np.diff(m.indptr), dtype=np.int32)
    rows = np.arange(ilower, ilower + n, dtype=np.int64)
    cols = np.ascontiguousarray(m.indices, dtype=np.int64) + jlower
    vals = np.ascontiguousarray(m.data, dtype=np.float64)
    ok = ok and L.HYPRE_IJMatrixSetValues(h, n, sizes.ctypes.data_as(C.POINTER(C.c_int)), rows.ctypes.data_as(ll), cols.ctypes.data_as(ll),
                                          vals.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ok = ok and L.HYPRE_IJMatrixAssemble(h) == 0
    if not ok:
        raise LibraryError("building an IJ matrix failed")
    return h


def ij_vector(values, jlower=0):
    """A numpy vector as an assembled HYPRE_IJVector (a handle, c_void_p) whose entries start at jlower"""
    L = lib()
    ll = C.POINTER(C.c_longlong)
    L.HYPRE_IJVectorCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.POINTER(C.c_void_p)]
    L.HYPRE_IJVectorSetObjectType.argtypes = [C.c_void_p, C.c_int]
    L.HYPRE_IJVectorInitialize.argtypes = L.HYPRE_IJVectorAssemble.argtypes = L.HYPRE_IJVectorDestroy.argtypes = [C.c_void_p]
    L.HYPRE_IJVectorSetValues.argtypes = [C.c_void_p, C.c_int, ll, C.POINTER(C.c_double)]
    v = np.ascontiguousarray(values, dtype=np.float64)
    idx = np.arange(jlower, jlower + v.size, dtype=np.int64)
    h = C.c_void_p()
    ok = L.HYPRE_IJVectorCreate(MPI_COMM_WORLD, jlower, jlower + v.size - 1, C.byref(h)) == 0
    ok = ok and L.HYPRE_IJVectorSetObjectType(h, 5555) == 0 and L.HYPRE_IJVectorInitialize(h) == 0
    ok = ok and L.HYPRE_IJVectorSetValues(h, v.size, idx.ctypes.data_as(ll), v.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ok = ok and L.HYPRE_IJVectorAssemble(h) == 0
    if not ok:
        raise LibraryError("building an IJ vector failed")
    return h


MEMORY_HOST, MEMORY_DEVICE = 0, 1  # HYPRE_MemoryLocation


def hypre_error_text():
    """the text of the last failed HYPRE_* call of this rank (HYPRE_DescribeError), cleared with the error flag"""
    L = lib()
    buf = C.create_string_buffer(128)
    L.HYPRE_DescribeError.argtypes = [C.c_int, C.c_char_p]
    L.HYPRE_DescribeError(L.HYPRE_GetError(), buf)
    L.HYPRE_ClearAllErrors()
    return buf.value.decode(errors="replace")


def _ij_check(code, what):
    if code:
        raise LibraryError(f"{what} failed: {hypre_error_text()}")


def _ij_device_sigs(L):
    vp = C.c_void_p
    L.HYPRE_IJMatrixCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.HYPRE_IJMatrixSetObjectType.argtypes = L.HYPRE_IJVectorSetObjectType.argtypes = [vp, C.c_int]
    L.HYPRE_IJMatrixInitialize_v2.argtypes = L.HYPRE_IJVectorInitialize_v2.argtypes = [vp, C.c_int]
    L.HYPRE_IJMatrixAssemble.argtypes = L.HYPRE_IJMatrixDestroy.argtypes = [vp]
    L.HYPRE_IJVectorAssemble.argtypes = L.HYPRE_IJVectorDestroy.argtypes = [vp]
    L.HYPRE_IJMatrixSetValues.argtypes = L.HYPRE_IJMatrixAddToValues.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.HYPRE_IJVectorCreate.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.HYPRE_IJVectorSetValues.argtypes = L.HYPRE_IJVectorAddToValues.argtypes = L.HYPRE_IJVectorGetValues.argtypes = [vp, C.c_int, vp, vp]
    L.HYPREDRV_AMD_IJVectorDevicePointer.argtypes = [vp, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int)]
    L.HYPREDRV_AMD_IJVectorDevicePointer.restype = C.c_uint32


def _count(a):
    """elements of a device array argument (DeviceBuffer, torch tensor, __cuda_array_interface__)"""
    if hasattr(a, "__cuda_array_interface__"):
        return int(np.prod(a.__cuda_array_interface__["shape"], dtype=np.int64))
    if hasattr(a, "numel"):
        return int(a.numel())
    return len(a)


def ij_matrix_device(ncols, rows, cols, vals, ilower, iupper, jlower, jupper, add=False, handle=None):
    """One HYPRE_IJMatrixSetValues (add: AddToValues) call with DEVICE arrays -- int32 ncols and int64 rows (one per row of the call),
    int64 cols and float64 vals (one per entry); DeviceBuffers, torch-ROCm tensors or anything with __cuda_array_interface__ /
    data_ptr(), passed without a copy -- on a matrix initialised with HYPRE_MEMORY_DEVICE.  handle=None creates that matrix for rows
    [ilower, iupper] and columns [jlower, jupper]; handle= stacks a further call on an open one.  Returns the handle, not assembled
    (ij_matrix_assemble).  A pointer of the wrong kind is undefined behaviour, as in hypre."""
    from ._lib import device_pointer
    L = lib()
    _ij_device_sigs(L)
    if handle is None:
        handle = C.c_void_p()
        _ij_check(L.HYPRE_IJMatrixCreate(MPI_COMM_WORLD, ilower, iupper, jlower, jupper, C.byref(handle)), "HYPRE_IJMatrixCreate")
        L.HYPRE_IJMatrixSetObjectType(handle, 5555)
        _ij_check(L.HYPRE_IJMatrixInitialize_v2(handle, MEMORY_DEVICE), "HYPRE_IJMatrixInitialize_v2")
    fn = L.HYPRE_IJMatrixAddToValues if add else L.HYPRE_IJMatrixSetValues
    _ij_check(fn(handle, _count(ncols), device_pointer(ncols), device_pointer(rows), device_pointer(cols), device_pointer(vals)),
              "HYPRE_IJMatrixAddToValues" if add else "HYPRE_IJMatrixSetValues")
    return handle


def ij_matrix_assemble(handle):
    """HYPRE_IJMatrixAssemble: the operator is built on the device from the stacked calls; returns the handle"""
    L = lib()
    _ij_device_sigs(L)
    _ij_check(L.HYPRE_IJMatrixAssemble(handle), "HYPRE_IJMatrixAssemble")
    return handle


def ij_vector_device(values, jlower, idx=None, add=False, handle=None, n=None):
    """One HYPRE_IJVectorSetValues (add: AddToValues) call with DEVICE arrays: float64 values, int64 idx (None: entries jlower, jlower
    + 1, ...).  handle=None creates a vector of len(values) entries starting at jlower (n: another length), initialised with
    HYPRE_MEMORY_DEVICE; handle= applies a further call.  Returns the handle, assembled."""
    from ._lib import device_pointer
    L = lib()
    _ij_device_sigs(L)
    cnt = _count(values)
    if handle is None:
        handle = C.c_void_p()
        nloc = cnt if n is None else int(n)
        _ij_check(L.HYPRE_IJVectorCreate(MPI_COMM_WORLD, jlower, jlower + nloc - 1, C.byref(handle)), "HYPRE_IJVectorCreate")
        L.HYPRE_IJVectorSetObjectType(handle, 5555)
        _ij_check(L.HYPRE_IJVectorInitialize_v2(handle, MEMORY_DEVICE), "HYPRE_IJVectorInitialize_v2")
    fn = L.HYPRE_IJVectorAddToValues if add else L.HYPRE_IJVectorSetValues
    _ij_check(fn(handle, cnt, device_pointer(idx), device_pointer(values)), "HYPRE_IJVectorAddToValues" if add else "HYPRE_IJVectorSetValues")
    _ij_check(L.HYPRE_IJVectorAssemble(handle), "HYPRE_IJVectorAssemble")
    return handle


def ij_vector_get_device(handle, idx=None, n=None):
    """HYPRE_IJVectorGetValues of a vector initialised with HYPRE_MEMORY_DEVICE into a new DeviceBuffer: the entries idx names (a
    device int64 array), or the first n owned ones (idx=None; n=None: all of them)."""
    from ._lib import DeviceBuffer, device_pointer
    L = lib()
    _ij_device_sigs(L)
    if idx is None and n is None:
        ll = C.POINTER(C.c_longlong)
        L.HYPRE_IJVectorGetLocalRange.argtypes = [C.c_void_p, ll, ll]
        lo, hi = C.c_longlong(), C.c_longlong()
        L.HYPRE_IJVectorGetLocalRange(handle, C.byref(lo), C.byref(hi))
        n = hi.value - lo.value + 1
    cnt = _count(idx) if idx is not None else int(n)
    out = DeviceBuffer.empty(cnt, np.float64)
    _ij_check(L.HYPRE_IJVectorGetValues(handle, cnt, device_pointer(idx), out.ptr), "HYPRE_IJVectorGetValues")
    return out


def vector_device_view(handle):
    """(device address, n) of the owned entries of an IJ vector handle -- HYPREDRV_AMD_IJVectorDevicePointer: read-only, valid until the
    vector is next modified or destroyed.  _lib.download_device(ptr, n) copies it to the host."""
    L = lib()
    _ij_device_sigs(L)
    p, n = C.POINTER(C.c_double)(), C.c_int()
    check(L.HYPREDRV_AMD_IJVectorDevicePointer(handle, C.byref(p), C.byref(n)))
    return C.cast(p, C.c_void_p).value or 0, n.value


class HypredrvError(LibraryError):
    def __init__(self, code, msg):
        super().__init__(f"HYPREDRV error 0x{code:08x}: {msg}")
        self.code = code


def check(code):
    if code:
        msg = lib().HYPREDRV_AMD_LastErrorMessage().decode()
        lib().HYPREDRV_ErrorCodeClear()
        raise HypredrvError(code, msg)


class Hypredrv:
    """Library-mode object, used like examples/src/C_laplacian/laplacian.c:331-468 uses HYPREDRV_t."""

    def __init__(self, yaml_text=None, library_mode=True, overrides=()):
        L = lib()
        check(L.HYPREDRV_Initialize())
        self.h = C.c_void_p()
        check(L.HYPREDRV_Create(MPI_COMM_WORLD, C.byref(self.h)))
        if library_mode:
            check(L.HYPREDRV_SetLibraryMode(self.h))
        if yaml_text is not None:
            self.parse(yaml_text, overrides)

    def parse(self, yaml_text, overrides=()):
        args = [yaml_text.encode()] + [o.encode() for o in overrides]
        argv = (C.c_char_p * len(args))(*args)
        check(lib().HYPREDRV_InputArgsParse(len(args), argv, self.h))

    def presets(self, solver="pcg", precon="poisson"):
        check(lib().HYPREDRV_InputArgsSetSolverPreset(self.h, solver.encode()))
        check(lib().HYPREDRV_InputArgsSetPreconPreset(self.h, precon.encode()))

    def set_matrix_csr(self, row_start, row_end, indptr, cols, data):
        if row_end == row_start - 1:  # a rank that owns nothing: the reference's entry refuses the range, the extension sets matrix AND rhs
            self._empty_block = True
            check(lib().HYPREDRV_AMD_LinearSystemSetEmptyBlock(self.h, row_start))
            return
        self._empty_block = False
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        cj = np.ascontiguousarray(cols, dtype=np.int64)
        v = np.ascontiguousarray(data, dtype=np.float64)
        ll = C.POINTER(C.c_longlong)
        check(lib().HYPREDRV_LinearSystemSetMatrixFromCSR(self.h, row_start, row_end, ip.ctypes.data_as(ll),
                                                          cj.ctypes.data_as(ll), v.ctypes.data_as(C.POINTER(C.c_double))))

    def set_rhs_array(self, row_start, row_end, values):
        if row_end == row_start - 1 and getattr(self, "_empty_block", False):
            return  # (set together with the empty matrix block)
        v = np.ascontiguousarray(values, dtype=np.float64)
        check(lib().HYPREDRV_LinearSystemSetRHSFromArray(self.h, row_start, row_end, v.ctypes.data_as(C.POINTER(C.c_double))))

    def set_laplacian7(self, n, P=(1, 1, 1), c=(1.0, 1.0, 1.0)):
        check(lib().HYPREDRV_AMD_LinearSystemSetLaplacian7pt(self.h, (C.c_int * 3)(*n), (C.c_int * 3)(*P), (C.c_double * 3)(*c)))

    def set_matrix(self, A):
        """an IJ matrix handle (ij_matrix); owned by the object unless it is in library mode"""
        check(lib().HYPREDRV_LinearSystemSetMatrix(self.h, A))

    def set_rhs(self, b):
        check(lib().HYPREDRV_LinearSystemSetRHS(self.h, b))

    def set_discrete_gradient(self, G):
        """the AMS discrete gradient, an IJ matrix handle or None"""
        check(lib().HYPREDRV_LinearSystemSetDiscreteGradient(self.h, G))

    def set_coordinates(self, x, y, z):
        """the AMS vertex coordinates, three IJ vector handles (or None)"""
        check(lib().HYPREDRV_LinearSystemSetCoordinates(self.h, x, y, z))

    def finish_system(self):
        check(lib().HYPREDRV_LinearSystemSetInitialGuess(self.h, None))
        check(lib().HYPREDRV_LinearSystemSetPrecMatrix(self.h, None))

    def solve(self):
        """ResetInitialGuess + Create + Setup + Apply + Destroy (laplacian.c:445-463)."""
        L = lib()
        check(L.HYPREDRV_LinearSystemResetInitialGuess(self.h))
        check(L.HYPREDRV_LinearSolverCreate(self.h))
        check(L.HYPREDRV_LinearSolverSetup(self.h))
        check(L.HYPREDRV_LinearSolverApply(self.h))
        out = self.last()
        check(L.HYPREDRV_LinearSolverDestroy(self.h))
        return out

    def create_and_setup(self):
        check(lib().HYPREDRV_LinearSolverCreate(self.h))
        check(lib().HYPREDRV_LinearSolverSetup(self.h))

    def apply(self, reset=True):
        if reset:
            check(lib().HYPREDRV_LinearSystemResetInitialGuess(self.h))
        check(lib().HYPREDRV_LinearSolverApply(self.h))
        return self.last()

    def apply_multi(self, k, b, x, ld, location=MEMORY_HOST, iters=None, final_rel=None):
        """HYPREDRV_AMD_LinearSolverApplyMulti as it is declared: b, x raw addresses (ints or None), iters / final_rel ctypes pointers"""
        check(lib().HYPREDRV_AMD_LinearSolverApplyMulti(self.h, k, location, b, x, ld, iters, final_rel))

    def solve_multi(self, B, X0=None, device=False, ld=None, k=None):
        """k <= 8 right-hand sides (the columns of B, n x k) through one pass over every operator, against what create_and_setup
        prepared.  X0: the initial guesses (zero by default); ld: the distance between two vectors in the arrays handed to the
        library (n by default).  device=True: B and X0 are device arrays (DeviceBuffer, torch-ROCm tensor) that hold k vectors one
        after the other, vector j at element j * ld (k: how many of them, all that B holds by default); X0 is overwritten with
        the solutions and returned as it is.  Returns (X, iters, final_rel)."""
        if device:
            from ._lib import device_pointer
            if X0 is None or ld is None:
                raise ValueError("solve_multi(device=True) needs X0 (in / out) and ld")
            k = _count(B) // int(ld) if k is None else int(k)
            it, fr = np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1))
            self.apply_multi(k, device_pointer(B), device_pointer(X0), int(ld), MEMORY_DEVICE, it.ctypes.data_as(C.POINTER(C.c_int)),
                             fr.ctypes.data_as(C.POINTER(C.c_double)))
            return X0, it[:k].copy(), fr[:k].copy()
        B = np.asarray(B, dtype=np.float64)
        B = B.reshape(-1, 1) if B.ndim == 1 else B
        n, k = B.shape
        ld = n if ld is None else int(ld)
        bt, xt = np.zeros((max(k, 1), ld)), np.zeros((max(k, 1), ld))
        bt[:k, :n] = B.T
        if X0 is not None:
            xt[:k, :n] = np.asarray(X0, dtype=np.float64).reshape(n, k).T
        it, fr = np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1))
        self.apply_multi(k, bt.ctypes.data, xt.ctypes.data, ld, MEMORY_HOST, it.ctypes.data_as(C.POINTER(C.c_int)),
                         fr.ctypes.data_as(C.POINTER(C.c_double)))
        return xt[:k, :n].T.copy(), it[:k].copy(), fr[:k].copy()

    def destroy_solver(self):
        check(lib().HYPREDRV_LinearSolverDestroy(self.h))

    def last(self):
        L = lib()
        it, cv = C.c_int(), C.c_int()
        rel, ts, tv = C.c_double(), C.c_double(), C.c_double()
        check(L.HYPREDRV_LinearSolverGetNumIter(self.h, C.byref(it)))
        check(L.HYPREDRV_LinearSolverGetConverged(self.h, C.byref(cv)))
        check(L.HYPREDRV_LinearSolverGetFinalRelativeResidualNorm(self.h, C.byref(rel)))
        check(L.HYPREDRV_LinearSolverGetSetupTime(self.h, C.byref(ts)))
        check(L.HYPREDRV_LinearSolverGetSolveTime(self.h, C.byref(tv)))
        return dict(iters=it.value, converged=bool(cv.value), final_rel=rel.value, setup_s=ts.value, solve_s=tv.value)

    def solution(self):
        p = C.POINTER(C.c_double)()
        n = C.c_longlong()
        check(lib().HYPREDRV_LinearSystemGetSolutionValues(self.h, C.byref(p)))
        check(lib().HYPREDRV_LinearSystemGetSolutionLength(self.h, C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[:n.value].copy()

    def solution_handle(self):
        """the solution as an IJ vector handle (HYPREDRV_LinearSystemGetSolution); vector_device_view(handle) reads it in HBM"""
        v = C.c_void_p()
        lib().HYPREDRV_LinearSystemGetSolution.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib().HYPREDRV_LinearSystemGetSolution.restype = C.c_uint32
        check(lib().HYPREDRV_LinearSystemGetSolution(self.h, C.byref(v)))
        return v

    def solution_norm(self, kind="L2"):
        v = C.c_double()
        check(lib().HYPREDRV_LinearSystemGetSolutionNorm(self.h, kind.encode(), C.byref(v)))
        return v.value

    def solve_phase_bytes(self):
        """(iteration, vcycle) bytes of this rank: each a pair (CSR figure, bytes in the formats read)."""
        it, vc = (C.c_double * 2)(), (C.c_double * 2)()
        check(lib().HYPREDRV_AMD_SolvePhaseBytes(self.h, it, vc))
        return (it[0], it[1]), (vc[0], vc[1])

    def residual_norms(self):
        """(r0, relative residual) of the last apply in full precision, and whether x is known to be the untouched zero fill now"""
        r0, rel, z = C.c_double(), C.c_double(), C.c_int()
        check(lib().HYPREDRV_AMD_LastResidualNorms(self.h, C.byref(r0), C.byref(rel), C.byref(z)))
        return r0.value, rel.value, bool(z.value)

    def probe_dominant_arm(self):
        """Time every Jacobi-sweep launch on this rank's largest plain-CSR operator; returns (level, rows, cols, nnz)."""
        lvl, dims = C.c_int(), (C.c_double * 3)()
        check(lib().HYPREDRV_AMD_ProbeDominant(self.h, 1, C.byref(lvl), dims, None, None))
        return lvl.value, int(dims[0]), int(dims[1]), int(dims[2])

    def probe_dominant_read(self):
        ms, n = C.c_double(), C.c_int()
        check(lib().HYPREDRV_AMD_ProbeDominant(self.h, 0, None, None, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stats_print(self):
        check(lib().HYPREDRV_StatsPrint(self.h))

    def close(self):
        if self.h:
            lib().HYPREDRV_Destroy(C.byref(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
