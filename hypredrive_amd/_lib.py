"""ctypes binding of the kernel-level C ABI (include/hypredrv_amd.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, "lib", "libhypredrv_amd.so")
_L = None


class LibraryError(RuntimeError):
    pass


class AmgParams(C.Structure):
    _fields_ = [("coarsen_type", C.c_int), ("interp_type", C.c_int), ("pmax", C.c_int),
                ("trunc_factor", C.c_double), ("strong_th", C.c_double),
                ("max_row_sum", C.c_double), ("max_coarse_size", C.c_int),
                ("min_coarse_size", C.c_int), ("max_levels", C.c_int),
                ("relax_down", C.c_int), ("relax_up", C.c_int), ("relax_coarse", C.c_int),
                ("sweeps_down", C.c_int), ("sweeps_up", C.c_int), ("sweeps_coarse", C.c_int),
                ("relax_weight", C.c_double), ("outer_weight", C.c_double),
                ("seed", C.c_uint64), ("num_functions", C.c_int),
                ("cheby_order", C.c_int), ("cheby_eig_est", C.c_int), ("cheby_variant", C.c_int), ("cheby_scale", C.c_int),
                ("cheby_fraction", C.c_double),
                ("smooth_num_levels", C.c_int), ("smooth_num_sweeps", C.c_int),
                ("ilu_tri_solve", C.c_int), ("ilu_lower_it", C.c_int), ("ilu_upper_it", C.c_int),
                ("restrict_type", C.c_int), ("restrict_strong_th", C.c_double), ("restrict_filter_th", C.c_double), ("relax_points", C.c_int),
                ("agg_p12_pmax", C.c_int), ("agg_p12_trunc_factor", C.c_double),
                ("smooth_type", C.c_int), ("fsai_num_levels", C.c_int), ("fsai_max_nnz_row", C.c_int), ("fsai_eig_max_iters", C.c_int),
                ("fsai_threshold", C.c_double),
                ("agg_num_levels", C.c_int), ("agg_num_paths", C.c_int), ("agg_interp_type", C.c_int),
                ("agg_pmax", C.c_int), ("agg_trunc_factor", C.c_double),
                ("blocks", C.c_int), ("block_part", C.POINTER(C.c_int64)), ("struct_size", C.c_int)]

    @staticmethod
    def default(**kw):
        p = AmgParams()
        load().hda_amg_default_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            if k == "block_part":
                if v is None:
                    continue
                keep = np.ascontiguousarray(v, dtype=np.int64)
                p._block_part_keep = keep  # (borrowed until the setup has read it)
                p.block_part = keep.ctypes.data_as(C.POINTER(C.c_int64))
                continue
            setattr(p, k, v)
        return p


class KrylovParams(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("rtol", C.c_double), ("atol", C.c_double),
                ("two_norm", C.c_int), ("krylov_dim", C.c_int)]

    @staticmethod
    def default(gmres=False, **kw):
        p = KrylovParams()
        load().hda_krylov_default_params(C.byref(p), 1 if gmres else 0)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p


class MgrLevelParams(C.Structure):
    _fields_ = [("n_f_labels", C.c_int), ("f_labels", C.POINTER(C.c_int)), ("interp_type", C.c_int), ("restrict_type", C.c_int),
                ("frelax_type", C.c_int), ("frelax_sweeps", C.c_int), ("grelax_type", C.c_int), ("grelax_sweeps", C.c_int),
                ("frelax_amg", C.POINTER(AmgParams)),
                ("ilu_tri_solve", C.c_int), ("ilu_lower_it", C.c_int), ("ilu_upper_it", C.c_int),
                ("coarse_ilu_max_iter", C.c_int), ("coarse_ilu_tri_solve", C.c_int), ("coarse_ilu_lower_it", C.c_int), ("coarse_ilu_upper_it", C.c_int),
                ("frelax_krylov", C.c_int), ("frelax_krylov_precond", C.c_int), ("frelax_kp", KrylovParams),
                ("coarse_krylov", C.c_int), ("coarse_krylov_precond", C.c_int), ("coarse_kp", KrylovParams),
                ("mgr_cycle", C.c_int), ("mgr_frelax_pos", C.c_int), ("mgr_gsmooth_pos", C.c_int), ("grelax_blocks", C.c_int),
                ("coarse_type", C.c_int), ("nonglk_max_elmts", C.c_int), ("coarse_th", C.c_double)]


def _signatures():
    """function -> (restype, argtypes) for every function include/hypredrv_amd.h declares, and for the test entries it does not"""
    P = C.POINTER
    I, D, S, VP, U64, I64 = C.c_int, C.c_double, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int64
    IP, DP, LP, LLP, MASK, OUT = P(I), P(D), P(I64), P(C.c_longlong), P(C.c_ubyte), P(VP)
    AMG, KRY = P(AmgParams), P(KrylovParams)
    interp = (I, [VP, MASK, IP, I, D, OUT])
    krylov = (I, [VP, VP, KRY, DP, DP, DP, IP, IP, DP])
    view = (I, [VP, I, OUT])
    declared = {
        "hda_last_error": (S, []), "hda_device_count": (I, []), "hda_device_name": (I, [S, I]), "hda_device_pci_bus_id": (I, [I, S, I]),
        "hda_device_sync": (I, []), "hda_marker": (I, [I]),
        "hda_amg_default_params": (None, [AMG]), "hda_krylov_default_params": (None, [KRY, I]),
        "hda_csr_create": (I, [I, I, LP, LP, DP, OUT]), "hda_csr_destroy": (I, [VP]), "hda_csr_dims": (I, [VP, IP, IP, IP]),
        "hda_csr_download": (I, [VP, IP, IP, DP]), "hda_lap7_create": (I, [IP, IP, IP, DP, OUT, DP]),
        "hda_spmv": (I, [VP, D, DP, D, DP]), "hda_relax": (I, [VP, I, D, I, DP, DP]), "hda_dot": (I, [I, DP, DP, DP]),
        "hda_l1_norms": (I, [VP, I, DP]),
        "hda_relax_blocks": (I, [VP, I, D, I, I, LP, DP, DP]), "hda_l1_norms_blocks": (I, [VP, I, I, LP, DP]),
        "hda_hmis_blocks": (I, [VP, MASK, I, LP, U64, I, IP]), "hda_cljp": (I, [VP, MASK, U64, I, I64, IP, IP]),
        "hda_rs_blocks": (I, [VP, MASK, I, LP, IP]), "hda_falgout_blocks": (I, [VP, MASK, I, LP, U64, I, IP, IP]),
        "hda_measure_rnd": (I, [I, U64, I, I64, DP]),
        "hda_strength": (I, [VP, D, D, MASK]), "hda_pmis": (I, [VP, MASK, U64, I, I64, IP]),
        "hda_interp_extpi": interp, "hda_interp_direct": interp, "hda_interp_mm_extpi": interp, "hda_interp_extended": interp,
        "hda_interp_mm_ext": interp, "hda_interp_standard": interp, "hda_interp_one_point": (I, [VP, MASK, IP, OUT]),
        "hda_rap": (I, [VP, VP, OUT]), "hda_air_restriction": (I, [VP, IP, I, D, D, OUT, LP]),
        "hda_second_strength": (I, [VP, MASK, IP, I, OUT]), "hda_coarsen_second_pass": (I, [VP, MASK, I, U64, I, IP]),
        "hda_interp_multipass": (I, [VP, MASK, IP, OUT]), "hda_truncate_rows": (I, [VP, I, D]),
        "hda_interp_agg_two_stage": (I, [VP, MASK, IP, IP, I, I, D, I, D, OUT, OUT, OUT]),
        "hda_transpose": (I, [VP, OUT]), "hda_spgemm": (I, [VP, VP, OUT]),
        "hda_spgemm_last_route": (I, [LP]), "hda_sort_rows_last_route": (I, [LP]),
        "hda_amg_create": (I, [AMG, VP, OUT]), "hda_amg_create_dof": (I, [AMG, VP, IP, OUT]), "hda_amg_destroy": (I, [VP]),
        "hda_ilu_create": (I, [VP, I, I, I, I, OUT]), "hda_ilu_create_blocks": (I, [VP, I, I, I, I, I, LP, OUT]),
        "hda_ilu_blocks": (I, [VP, I]), "hda_ilu_factors": view,
        "hda_schwarz_create": (I, [VP, I, I, I, I, LP, I, D, OUT]), "hda_schwarz_domains": (I, [VP, IP, IP, IP]),
        "hda_schwarz_info": (I, [VP, LP, DP]),
        "hda_fsai_create": (I, [VP, I, D, I, I, I, I, LP, OUT]), "hda_fsai_factor": view, "hda_fsai_info": (I, [VP, I, LP, DP]),
        "hda_precond_time": (I, [VP, I, DP]),
        "hda_ams_default_amg_params": (None, [AMG, I]), "hda_ams_create": (I, [VP, VP, DP, DP, DP, I, I, I, D, I, AMG, AMG, OUT]),
        "hda_ams_matrix": view, "hda_ams_info": (I, [VP, LP, DP]),
        "hda_mgr_create": (I, [VP, IP, I, P(MgrLevelParams), AMG, I, OUT]), "hda_mgr_matrix": (I, [VP, I, I, OUT]),
        "hda_mgr_blk_inverses": (I, [VP, I, I, DP, IP, IP]),
        "hda_amg_num_levels": (I, [VP]), "hda_amg_level_matrix": (I, [VP, I, I, OUT]), "hda_amg_level_cf": (I, [VP, I, IP]),
        "hda_amg_fold_sweep": (I, [VP, I, DP, DP, DP, DP, DP]), "hda_amg_blocks": (I, [VP]), "hda_amg_level_blocks": (I, [VP, I, LP]),
        "hda_amg_complexities": (I, [VP, DP, DP]), "hda_amg_vcycle_bytes": (D, [VP]), "hda_amg_vcycle": (I, [VP, DP, DP]),
        "hda_pcg": krylov, "hda_gmres": krylov, "hda_fgmres": krylov, "hda_bicgstab": krylov,
        "hda_spmm": (I, [VP, I, I, D, D, DP, DP, DP, DP, DP, DP, DP]), "hda_multi_blas": (I, [I, I, I, DP, DP, IP, DP, DP, DP, DP, DP]),
        "hda_amg_vcycle_multi": (I, [VP, I, DP, DP]), "hda_pcg_multi": (I, [VP, VP, KRY, I, DP, DP, DP, IP, IP, DP]),
        "hda_time_kernel_multi": (I, [I, VP, VP, I, I, DP, DP]),
        "hda_time_kernel": (I, [I, VP, VP, I, DP, DP]), "hda_set_overlap": (None, [I]), "hda_last_precond_calls": (I, []),
        "hda_solve_device": (I, [VP, VP, KRY, I, DP, I, DP, IP, DP, DP, DP, DP]),
        "hda_pcg_iteration_bytes": (D, [VP]), "hda_format_bytes": (I, [VP, VP, DP, DP, DP, IP]),
        "hda_csr_form": (I, [VP, I, IP]), "hda_spmv_mode": (I, [VP, I, I, D, D, DP, DP, DP, DP, DP, DP, DP, DP, DP, IP]),
        "hda_borrow_hypredrv": (I, [VP, OUT, OUT]), "hda_amd_partitioned_levels": (I, [VP]), "hda_amd_hierarchy_levels": (I, [VP]),
        "hda_halo_plan_host": (I, [I, LLP, LLP, I, IP, IP, IP, I, IP]),
        "hda_dev_alloc": (I, [I64, OUT]), "hda_dev_free": (I, [VP]), "hda_dev_upload": (I, [VP, VP, I64]),
        "hda_dev_download": (I, [VP, VP, I64]), "hda_borrow_ij_matrix": (I, [VP, OUT]), "hda_ij_ghost_gids": (I, [VP, LLP, I, IP]),
        "hda_ij_last_assembly": (I, [DP]),
        "hda_probe_spmv": (I, [VP, I]), "hda_probe_read": (I, [DP, IP]), "hda_probe_add": (I, [VP, I, IP]),
        "hda_probe_read_id": (I, [I, DP, IP]),
        "hda_comm_stats": (I, [DP, I]), "hda_comm_name": (S, []), "hda_comm_size": (I, []), "hda_comm_selftest": (I, []),
        "hda_check_row_total": (I, [C.c_longlong, I]),
        "hda_memory_stats": (I, [DP, DP]), "hda_memory_cached": (D, []), "hda_memory_driver_stats": (I, [DP, I]), "hda_memory_trim": (I, []),
    }
    undeclared = {"hda_amg_rebind": (I, [VP, VP]), "hda_amg_level0_sweep": (I, [VP, I, DP, DP, DP, DP, IP])}
    return declared, undeclared


_DECLARED, _UNDECLARED = _signatures()
SYMBOLS = list(_DECLARED)  # (tests/test_cabi_symbols.py compares them with the header)


TESTRANKS_SYMBOLS = ["hda_thread_ranks_lap7", "hda_thread_world_create", "hda_thread_world_join", "hda_thread_world_leave",
                     "hda_thread_world_destroy", "hda_testranks_selftest"]
_TESTRANKS_PATH = os.path.join(os.path.dirname(_LIBPATH), "libhypredrv_amd_testranks.so")
_T = None


def load_testranks():
    """The test seam "ranks as threads of one process" (include/hypredrv_amd_testranks.h): its own small library on top of the
    product library, which is loaded first so that both share one instance of it."""
    global _T
    if _T is None:
        load()
        if not os.path.exists(_TESTRANKS_PATH):
            raise LibraryError(f"{_TESTRANKS_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _T = C.CDLL(_TESTRANKS_PATH)
    return _T


def testranks_selftest(what, cache_gb=8.0):
    """include/hypredrv_amd_testranks.h hda_testranks_selftest: (ok, the ranks' messages)"""
    T = load_testranks()
    T.hda_testranks_selftest.argtypes = [C.c_int, C.c_double, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(4096)
    rc = T.hda_testranks_selftest(int(what), float(cache_gb), buf, 4096)
    return rc == 0, buf.value.decode(errors="replace")


def load():
    """Load libhypredrv_amd.so; raises (never falls back) when it is missing."""
    global _L
    if _L is not None:
        return _L
    if not os.path.exists(_LIBPATH):
        raise LibraryError(
            f"{_LIBPATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the MI355X solve path has no CPU fallback)")
    L = C.CDLL(_LIBPATH)
    for name, (restype, argtypes) in {**_DECLARED, **_UNDECLARED}.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _L = L
    return L


def _check(rc):
    if rc != 0:
        raise LibraryError(f"libhypredrv_amd error {rc}: {load().hda_last_error().decode()}")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


# staging of the kernel-level entries: the C side reads exactly nnz mask bytes / nrows markers, so the arrays go as they are (the
# pointer keeps its array alive)
def _mask(smask):
    return np.ascontiguousarray(smask, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_ubyte))


def _marker(cf):
    return _ip(np.ascontiguousarray(cf, dtype=np.int32))


def _blocks(part):
    """(nblk, pointer to the nblk + 1 int64 row starts)"""
    pt = np.ascontiguousarray(part, dtype=np.int64)
    return len(pt) - 1, pt.ctypes.data_as(C.POINTER(C.c_int64))


def _blocks_or(blocks, block_part):
    """(blocks, NULL) unless block_part names the row starts"""
    return (blocks, None) if block_part is None else _blocks(block_part)


def _cols(a):
    """a multivector as a 2-d float64 array, one column per vector (a 1-d array is one column)"""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def _new_csr(fn, *args, **how):
    """call an entry whose last argument is the new matrix handle; how: owned=False, keep=... for a borrowed view"""
    out = C.c_void_p()
    _check(fn(*args, C.byref(out)))
    return Csr(out, **how)


def device_count():
    return load().hda_device_count()


def device_name():
    buf = C.create_string_buffer(256)
    _check(load().hda_device_name(buf, 256))
    return buf.value.decode()


class Csr:
    """CSR block resident in HBM."""

    def __init__(self, handle, owned=True, keep=None):
        self.h = handle
        self.owned = owned
        self._keep = keep
        self.rhs = None

    def __del__(self):
        if getattr(self, "owned", False) and self.h:
            load().hda_csr_destroy(self.h)
            self.h = None

    @staticmethod
    def from_arrays(nrows, ncols, rowptr, cols, vals):
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        cj = np.ascontiguousarray(cols, dtype=np.int64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        return _new_csr(load().hda_csr_create, nrows, ncols, rp.ctypes.data_as(C.POINTER(C.c_int64)), cj.ctypes.data_as(C.POINTER(C.c_int64)), _dp(v))

    @staticmethod
    def from_scipy(m):
        m = m.tocsr()
        return Csr.from_arrays(m.shape[0], m.shape[1], m.indptr, m.indices, m.data)

    @property
    def dims(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(load().hda_csr_dims(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    nrows = property(lambda s: s.dims[0])
    ncols = property(lambda s: s.dims[1])
    nnz = property(lambda s: s.dims[2])

    def download(self):
        n, m, nnz = self.dims
        rp = np.zeros(n + 1, dtype=np.int32)
        cj = np.zeros(nnz, dtype=np.int32)
        v = np.zeros(nnz, dtype=np.float64)
        _check(load().hda_csr_download(self.h, _ip(rp), _ip(cj), _dp(v)))
        return rp, cj, v

    def to_scipy(self):
        import scipy.sparse as sp
        rp, cj, v = self.download()
        n, m, _ = self.dims
        return sp.csr_matrix((v, cj, rp), shape=(n, m))

    def spmv(self, x, alpha=1.0, beta=0.0, y=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.nrows) if y is None else np.ascontiguousarray(y, dtype=np.float64).copy()
        _check(load().hda_spmv(self.h, alpha, _dp(x), beta, _dp(y)))
        return y

    def spmm(self, X, mode="plain", alpha=1.0, beta=0.0, Yin=None, B=None, dinv=None, W=None, Y=None):
        """One batched product on k <= 8 columns (X: ncols x k; Yin, B, W: nrows x k; dinv: nrows), a SPMM_MODES name: plain Y = alpha
        A X + beta Yin, resid Y = B - A X, jacobi Y = X + dinv * (B - A X).  Y: what the output starts from (rows the product does
        not write come back unchanged).  Returns (Y, dots): Y nrows x k, dots the k values <W_j, Y_j> or None without W."""
        X = _cols(X)
        k = X.shape[1]
        n = self.nrows
        Yin, B, W = (None if v is None else _cols(v) for v in (Yin, B, W))
        out = np.zeros((k, n)) if Y is None else np.ascontiguousarray(np.asarray(Y, dtype=np.float64).T).copy()
        dots = np.zeros(max(k, 1))
        p = lambda v: None if v is None else _dp(np.ascontiguousarray(v.T))
        dv = None if dinv is None else np.ascontiguousarray(dinv, dtype=np.float64)
        _check(load().hda_spmm(self.h, SPMM_MODES[mode], k, alpha, beta, p(X), p(Yin), p(B), None if dv is None else _dp(dv), p(W), _dp(out),
                               _dp(dots) if W is not None else None))
        return out.T.copy(), (dots[:k].copy() if W is not None else None)

    def relax(self, b, x, relax_type=18, weight=1.0, sweeps=1):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        _check(load().hda_relax(self.h, relax_type, weight, sweeps, _dp(b), _dp(x)))
        return x

    def l1_norms(self, option=1):
        out = np.zeros(self.nrows)
        _check(load().hda_l1_norms(self.h, option, _dp(out)))
        return out

    # the row-block forms (part: V + 1 row starts) = the reference at np = V
    def relax_blocks(self, b, x, part, relax_type=13, weight=1.0, sweeps=1):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        _check(load().hda_relax_blocks(self.h, relax_type, weight, sweeps, *_blocks(part), _dp(b), _dp(x)))
        return x

    def l1_norms_blocks(self, option, part):
        out = np.zeros(self.nrows)
        _check(load().hda_l1_norms_blocks(self.h, option, *_blocks(part), _dp(out)))
        return out

    def hmis_blocks(self, smask, part, seed=2747, level=0):
        cf = np.zeros(self.nrows, dtype=np.int32)
        _check(load().hda_hmis_blocks(self.h, _mask(smask), *_blocks(part), seed, level, _ip(cf)))
        return cf

    # coarsen types 0 / 1 / 6; last_rounds: the CLJP rounds of the latest cljp / falgout_blocks call
    def cljp(self, smask, seed=2747, level=0, row_offset=0):
        cf = np.zeros(self.nrows, dtype=np.int32)
        rounds = C.c_int(0)
        _check(load().hda_cljp(self.h, _mask(smask), seed, level, row_offset, _ip(cf), C.byref(rounds)))
        self.last_rounds = rounds.value
        return cf

    def rs_blocks(self, smask, part=None):
        cf = np.zeros(self.nrows, dtype=np.int32)
        _check(load().hda_rs_blocks(self.h, _mask(smask), *_blocks([0, self.nrows] if part is None else part), _ip(cf)))
        return cf

    def falgout_blocks(self, smask, part=None, seed=2747, level=0):
        cf = np.zeros(self.nrows, dtype=np.int32)
        rounds = C.c_int(0)
        _check(load().hda_falgout_blocks(self.h, _mask(smask), *_blocks([0, self.nrows] if part is None else part), seed, level, _ip(cf),
                                         C.byref(rounds)))
        self.last_rounds = rounds.value
        return cf

    def strength(self, theta=0.25, max_row_sum=0.9):
        sm = np.zeros(self.nnz, dtype=np.uint8)
        _check(load().hda_strength(self.h, theta, max_row_sum, sm.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return sm

    def pmis(self, smask, seed=2747, level=0, row_offset=0):
        cf = np.zeros(self.nrows, dtype=np.int32)
        _check(load().hda_pmis(self.h, _mask(smask), seed, level, row_offset, _ip(cf)))
        return cf

    def interp_extpi(self, smask, cf, pmax=4, trunc_factor=0.0):
        return _new_csr(load().hda_interp_extpi, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def interp_mm_extpi(self, smask, cf, pmax=4, trunc_factor=0.0):
        """interpolation type 17 (mm-ext+i): the matrix-matrix form of extended+i"""
        return _new_csr(load().hda_interp_mm_extpi, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def interp_extended(self, smask, cf, pmax=4, trunc_factor=0.0):
        """interpolation type 14 (extended): extended+i without the point itself in its strong F neighbours' denominators"""
        return _new_csr(load().hda_interp_extended, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def interp_mm_ext(self, smask, cf, pmax=4, trunc_factor=0.0):
        """interpolation type 16 (mm_extended): mm-ext+i with s_ki := 0"""
        return _new_csr(load().hda_interp_mm_ext, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def interp_one_point(self, smask, cf):
        """interpolation type 100 (one_point): weight 1 towards the strong C neighbour of largest |a_ij|"""
        return _new_csr(load().hda_interp_one_point, self.h, _mask(smask), _marker(cf))

    def interp_standard(self, smask, cf, pmax=4, trunc_factor=0.0):
        """interpolation type 8 (standard): strong F neighbours eliminated through their own rows, direct interpolation on the result"""
        return _new_csr(load().hda_interp_standard, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def interp_direct(self, smask, cf, pmax=4, trunc_factor=0.0):
        """interpolation type 3 (direct_sep_weights)"""
        return _new_csr(load().hda_interp_direct, self.h, _mask(smask), _marker(cf), pmax, trunc_factor)

    def second_strength(self, smask, cf, num_paths=1):
        """aggressive coarsening: strong connections of distance <= 2 among the C points of cf (values = number of paths)"""
        return _new_csr(load().hda_second_strength, self.h, _mask(smask), _marker(cf), num_paths)

    def coarsen_second_pass(self, smask, cf, num_paths=1, seed=2747, level=0):
        """aggressive coarsening: the second PMIS pass; returns the updated C/F marker"""
        cfa = np.array(cf, dtype=np.int32)  # (a copy: the pass updates it in place)
        _check(load().hda_coarsen_second_pass(self.h, _mask(smask), num_paths, seed, level, _ip(cfa)))
        return cfa

    def interp_multipass(self, smask, cf):
        """aggressive coarsening: multipass interpolation (aggressive.prolongation_type 4)"""
        return _new_csr(load().hda_interp_multipass, self.h, _mask(smask), _marker(cf))

    def interp_agg_two_stage_parts(self, smask, cf1, cf2, plus_i=False, p12_pmax=0, p12_tf=0.0, pmax=0, tf=0.0):
        """aggressive.prolongation_type 5 (plus_i False: mm_extended) / 6 (True: mm_extended+i): (P1, P2, P) with P = P1 P2.  cf1: the
        splitting after the first coarsening pass, cf2: after coarsen_second_pass; P1 (n x |C1|) is truncated by p12_pmax / p12_tf,
        P2 (|C1| x |C2|) by pmax / tf."""
        o1, o2, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(load().hda_interp_agg_two_stage(self.h, _mask(smask), _marker(cf1), _marker(cf2), 1 if plus_i else 0,
                                               int(p12_pmax), float(p12_tf), int(pmax), float(tf), C.byref(o1), C.byref(o2), C.byref(o)))
        return Csr(o1), Csr(o2), Csr(o)

    def interp_agg_second_stage(self, smask, cf1, cf2, plus_i=False, pmax=0, tf=0.0):
        """P2 alone (only the |C1| rows of the second stage are built)"""
        o2 = C.c_void_p()
        _check(load().hda_interp_agg_two_stage(self.h, _mask(smask), _marker(cf1), _marker(cf2), 1 if plus_i else 0,
                                               0, 0.0, int(pmax), float(tf), None, C.byref(o2), None))
        return Csr(o2)

    def interp_agg_two_stage(self, smask, cf1, cf2, plus_i=False, p12_pmax=0, p12_tf=0.0, pmax=0, tf=0.0):
        """the product P of interp_agg_two_stage_parts"""
        return self.interp_agg_two_stage_parts(smask, cf1, cf2, plus_i, p12_pmax, p12_tf, pmax, tf)[2]

    def truncate_rows(self, pmax=0, trunc_factor=0.0):
        """hypre_BoomerAMGInterpTruncation on the finished rows of this interpolation matrix, in place"""
        _check(load().hda_truncate_rows(self.h, pmax, trunc_factor))
        return self

    def rap(self, P):
        return _new_csr(load().hda_rap, self.h, P.h)

    def transpose(self):
        return _new_csr(load().hda_transpose, self.h)

    def matmul(self, Y):
        return _new_csr(load().hda_spgemm, self.h, Y.h)


SPGEMM_PATHS = ("none", "esc", "hash")
SPGEMM_WHY_HASH = ("none", "empty input", "row longer than 4096 products", "scratch budget", "row-field overflow")
SORT_ROUTES = ("none", "insertion", "wave", "segmented")


def spgemm_last_route():
    """hda_spgemm_last_route: the route of this thread's last sparse product (Csr.matmul, the second product of Csr.rap, the last of
    a setup).  capacity, threads and nchunks are 0 on the hash path, batches 0 on the LDS path."""
    o = (C.c_int64 * 8)()
    _check(load().hda_spgemm_last_route(o))
    return {"path": SPGEMM_PATHS[o[0]], "why_hash": SPGEMM_WHY_HASH[o[1]], "capacity": o[2], "threads": o[3],
            "nchunks": o[4], "maxnp": o[5], "total": o[6], "batches": o[7]}


def sort_rows_last_route():
    """hda_sort_rows_last_route: "none", "insertion", "wave" or "segmented" -- the last row sort of this thread (Csr.from_arrays,
    Csr.transpose)"""
    r = C.c_int64()
    _check(load().hda_sort_rows_last_route(C.byref(r)))
    return SORT_ROUTES[r.value]


def lap7(nx, ny, nz, c=(1.0, 1.0, 1.0), want_rhs=True):
    """7-pt Laplacian generated in HBM (examples/src/C_laplacian/laplacian.c:719-921)."""
    n = (C.c_int * 3)(nx, ny, nz)
    P = (C.c_int * 3)(1, 1, 1)
    pc = (C.c_int * 3)(0, 0, 0)
    cc = (C.c_double * 3)(*c)
    out = C.c_void_p()
    rhs = np.zeros(nx * ny * nz) if want_rhs else None
    _check(load().hda_lap7_create(n, P, pc, cc, C.byref(out), _dp(rhs) if want_rhs else None))
    A = Csr(out)
    A.rhs = rhs
    return A


class Amg:
    def __init__(self, A, params=None, dof=None):
        self.A = A
        self.params = params if params is not None else AmgParams.default()
        self.h = C.c_void_p()
        if dof is None:
            _check(load().hda_amg_create(C.byref(self.params), A.h, C.byref(self.h)))
        else:
            _check(load().hda_amg_create_dof(C.byref(self.params), A.h, _marker(dof), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    @property
    def num_levels(self):
        return load().hda_amg_num_levels(self.h)

    def level_matrix(self, level, which=0):
        return _new_csr(load().hda_amg_level_matrix, self.h, level, which, owned=False, keep=self)

    def fold_sweep(self, level, dinv, t, e, u):
        """The folded up-leg sweep of a folded level as the cycle launches it: (u + dinv * t) + Pt e, Pt = level_matrix(level, 3)."""
        dinv, t, e, u = (np.ascontiguousarray(v, dtype=np.float64) for v in (dinv, t, e, u))
        M = self.level_matrix(level, 3)
        assert dinv.size == t.size == u.size == M.nrows and e.size == M.ncols
        out = np.zeros(M.nrows)
        _check(load().hda_amg_fold_sweep(self.h, level, _dp(dinv), _dp(t), _dp(e), _dp(u), _dp(out)))
        return out

    def level0_sweep(self, b, x, direction=0, want_dot=False):
        """One Jacobi sweep on level 0 as the cycle launches it: (x + dinv (b - A x), <b, out> or None, divisors read by row class?)."""
        b, x = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, x))
        out, dot, by_class = np.zeros_like(b), C.c_double(), C.c_int()
        _check(load().hda_amg_level0_sweep(self.h, direction, _dp(b), _dp(x), _dp(out), C.byref(dot) if want_dot else None, C.byref(by_class)))
        return out, (dot.value if want_dot else None), bool(by_class.value)

    def rebind(self, A):
        """Level 0 on another matrix of the same size; divisors and coarse levels are kept (preconditioner reuse)."""
        _check(load().hda_amg_rebind(self.h, A.h))
        self.A = A

    def ilu_factors(self, level):
        """Factors of the complex smoother (amg.smoother.type ilu) of a level."""
        return _new_csr(load().hda_ilu_factors, self.h, level, owned=False, keep=self)

    def fsai_factor(self, level):
        """G of the static FSAI smoother (amg.smoother.type fsai) of a level."""
        return _new_csr(load().hda_fsai_factor, self.h, level, owned=False, keep=self)

    def fsai_info(self, level):
        return _fsai_info(self.h, level)

    def level_cf(self, level):
        n = self.level_matrix(level, 0).nrows
        cf = np.zeros(n, dtype=np.int32)
        _check(load().hda_amg_level_cf(self.h, level, _ip(cf)))
        return cf

    @property
    def blocks(self):
        """row blocks the setup worked with (AmgParams.blocks resolved; 1 = none)"""
        return load().hda_amg_blocks(self.h)

    def level_blocks(self, level):
        out = np.zeros(max(self.blocks, 1) + 1, dtype=np.int64)
        _check(load().hda_amg_level_blocks(self.h, level, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    @property
    def complexities(self):
        g, o = C.c_double(), C.c_double()
        _check(load().hda_amg_complexities(self.h, C.byref(g), C.byref(o)))
        return g.value, o.value

    @property
    def vcycle_bytes(self):
        return load().hda_amg_vcycle_bytes(self.h)

    def vcycle(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        _check(load().hda_amg_vcycle(self.h, _dp(b), _dp(x)))
        return x

    def vcycle_multi(self, B):
        """One V-cycle from a zero guess on the k <= 8 columns of B (n x k) in one pass over every operator; returns X (n x k)."""
        B = _cols(B)
        k = B.shape[1]
        bt = np.ascontiguousarray(B.T)
        xt = np.zeros_like(bt)
        _check(load().hda_amg_vcycle_multi(self.h, k, _dp(bt), _dp(xt)))
        return xt.T.copy()


MGR_INTERP = {"injection": 0, "l1-jacobi": 1, "jacobi": 2, "blk-jacobi": 12}
MGR_COARSE = {"rap": 0, "galerkin": 0, "non-galerkin": 1}
MGR_RESTRICT = {"injection": 0, "jacobi": 2, "columped": 14}
MGR_FRELAX = {"jacobi": 7, "single": 7, "l1-jacobi": 18, "amg": 2, "ilu": 32}
MGR_GRELAX = {"none": -1, "h-fgs": 3, "h-bgs": 4, "h-ssor": 6, "l1-hfgs": 13, "l1-hbgs": 14, "l1-hsgs": 88, "ilu": 16}

MGR_KRYLOV = {"pcg": 1, "gmres": 2, "fgmres": 3, "bicgstab": 4}


def _mgr_nested(entry, lv):
    """nested Krylov components of a level dict: f_krylov / coarsest_krylov = dict(method=..., precond=True, **krylov params)"""
    for key, pre in (("f_krylov", "frelax"), ("coarsest_krylov", "coarse")):
        nk = lv.get(key)
        if not nk:
            continue
        kw = {k: v for k, v in nk.items() if k not in ("method", "precond")}
        kp = getattr(entry, pre + "_kp")
        for k, v in {**dict(max_iter=100, rtol=1e-6, atol=0.0, two_norm=1, krylov_dim=30), **kw}.items():
            setattr(kp, k, v)
        setattr(entry, pre + "_krylov", MGR_KRYLOV[nk.get("method", "gmres")])
        setattr(entry, pre + "_krylov_precond", 1 if nk.get("precond", True) else 0)
    cyc = lv.get("cycle")  # on the last level: "v(1,0)" (default), "v(0,1)", "v(1,1)", "w", "w(0,1)", "w(1,1)"
    if cyc:
        entry.mgr_cycle = 2 if cyc.startswith("w") else 1
        pos = {"": 1, "(1,0)": 1, "(0,1)": 2, "(1,1)": 3}[cyc[1:]]
        entry.mgr_frelax_pos = entry.mgr_gsmooth_pos = pos


class Mgr:
    """'preconditioner: mgr': multigrid reduction by dof labels; levels = list of dicts with the YAML keys of
    mgr.level.N (f_dofs, prolongation_type, restriction_type, f_relaxation, g_relaxation [, f_sweeps, g_sweeps]).
    Usable as amg= in pcg()/gmres()/fgmres()/bicgstab()."""

    def __init__(self, A, labels, levels, coarse_params=None, max_iter=1, coarsest="amg"):
        self.A = A
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.params = coarse_params if coarse_params is not None else AmgParams.default()
        arr = (MgrLevelParams * max(len(levels), 1))()
        self._keep = []
        for k, lv in enumerate(levels):
            f = np.ascontiguousarray(lv["f_dofs"], dtype=np.int32)
            self._keep.append(f)
            arr[k].n_f_labels = len(f)
            arr[k].f_labels = f.ctypes.data_as(C.POINTER(C.c_int))
            arr[k].interp_type = MGR_INTERP[lv.get("prolongation_type", "injection")]
            arr[k].restrict_type = MGR_RESTRICT[lv.get("restriction_type", "injection")]
            arr[k].frelax_type = MGR_FRELAX[lv.get("f_relaxation", "jacobi")]
            arr[k].frelax_sweeps = lv.get("f_sweeps", 1)
            arr[k].grelax_type = MGR_GRELAX[lv.get("g_relaxation", "none")]
            arr[k].grelax_sweeps = lv.get("g_sweeps", 1)
            arr[k].coarse_type = MGR_COARSE[lv.get("coarse_level_type", "rap")]
            arr[k].nonglk_max_elmts = lv.get("nonglk_max_elmts", 1)   # hypre's default (non-galerkin only)
            arr[k].coarse_th = lv.get("coarse_th", 0.0)
            arr[k].grelax_blocks = lv.get("g_blocks", 1)   # row blocks of the hybrid Gauss-Seidel global relaxation (the reference at np = V)
            if lv.get("f_amg") is not None:   # AmgParams of 'f_relaxation: {amg: {...}}'
                self._keep.append(lv["f_amg"])
                arr[k].frelax_amg = C.pointer(lv["f_amg"])
            ilu = lv.get("ilu", {})
            arr[k].ilu_tri_solve, arr[k].ilu_lower_it, arr[k].ilu_upper_it = ilu.get("tri_solve", 1), ilu.get("lower_jac_iters", 5), ilu.get("upper_jac_iters", 5)
            cil = lv.get("coarsest_ilu", {})
            arr[k].coarse_ilu_max_iter, arr[k].coarse_ilu_tri_solve = cil.get("max_iter", 1), cil.get("tri_solve", 1)
            arr[k].coarse_ilu_lower_it, arr[k].coarse_ilu_upper_it = cil.get("lower_jac_iters", 5), cil.get("upper_jac_iters", 5)
            _mgr_nested(arr[k], lv)
        self.nlevels = len(levels)
        self.h = C.c_void_p()
        _check(load().hda_mgr_create(A.h, _ip(self.labels), len(levels), arr, C.byref(self.params) if coarsest == "amg" else None,
                                     max_iter, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    def matrix(self, level, which=0):
        return _new_csr(load().hda_mgr_matrix, self.h, level, which, owned=False, keep=self)

    def block_inverses(self, level, tier=0):
        """F-block inverses of a reduction level as an array (nblk, b, b), and nf (the short last block: its top-left corner)"""
        b, nf = C.c_int(), C.c_int()
        _check(load().hda_mgr_blk_inverses(self.h, level, tier, None, C.byref(b), C.byref(nf)))
        if b.value == 0:
            return np.zeros((0, 0, 0)), 0
        nblk = -(-nf.value // b.value)
        out = np.zeros(nblk * b.value * b.value)
        _check(load().hda_mgr_blk_inverses(self.h, level, tier, _dp(out), C.byref(b), C.byref(nf)))
        return out.reshape(nblk, b.value, b.value), nf.value

    def vcycle(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        _check(load().hda_amg_vcycle(self.h, _dp(b), _dp(x)))
        return x


class Ilu:
    """'preconditioner: ilu': block-Jacobi ILU(0) of A's diagonal block; usable as amg= in pcg()/gmres()."""

    def __init__(self, A, max_iter=1, tri_solve=1, lower_it=5, upper_it=5, blocks=1, block_part=None):
        """blocks: V contiguous row blocks = bj-iluk at np = V (1 one block, 0 the setup's choice); block_part: V + 1 row starts"""
        self.A = A
        self.h = C.c_void_p()
        if blocks == 1 and block_part is None:
            _check(load().hda_ilu_create(A.h, max_iter, tri_solve, lower_it, upper_it, C.byref(self.h)))
        else:
            _check(load().hda_ilu_create_blocks(A.h, max_iter, tri_solve, lower_it, upper_it, *_blocks_or(blocks, block_part), C.byref(self.h)))

    @property
    def blocks(self):
        return load().hda_ilu_blocks(self.h, -1)

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    @property
    def factors(self):
        return _new_csr(load().hda_ilu_factors, self.h, -1, owned=False, keep=self)

    def apply(self, r):
        """One application from a zero guess (max_iter iterations x += M^-1 (r - A x))."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(load().hda_amg_vcycle(self.h, _dp(r), _dp(z)))
        return z


SCHWARZ_VARIANTS = {"ras": 0, "ras-iluk": 0, "as": 1, "as-iluk": 1}


class Schwarz:
    """'preconditioner: schwarz': restricted (ras) or additive (as) Schwarz on V row blocks grown by `overlap` layers of A's stored
    pattern, ILU(fill) subdomain solves; usable as amg= in pcg()/gmres()/fgmres()/bicgstab()."""

    def __init__(self, A, variant="ras", overlap=1, fill=0, blocks=1, block_part=None, max_iter=1, weight=1.0):
        """blocks: 1 one block, 0 the setup's choice, V the even split unless block_part names the V + 1 row starts"""
        self.A = A
        self.h = C.c_void_p()
        _check(load().hda_schwarz_create(A.h, SCHWARZ_VARIANTS[variant] if isinstance(variant, str) else int(variant), overlap, fill,
                                         *_blocks_or(blocks, block_part), max_iter, weight, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    def info(self):
        """dict: n_ext, nnz_factors, longest_row, global_rows (rows on the global-memory symbolic path), lds_capacity, nnz_A, setup_ms"""
        v, ms = (C.c_int64 * 6)(), (C.c_double * 4)()
        _check(load().hda_schwarz_info(self.h, v, ms))
        return dict(n_ext=v[0], nnz_factors=v[1], longest_row=v[2], global_rows=v[3], lds_capacity=v[4], nnz_A=v[5],
                    setup_ms=dict(expansion=ms[0], extraction=ms[1], symbolic=ms[2], numeric=ms[3]))

    def domains(self):
        """(dom_ptr, dom_rows): subdomain b holds the global rows dom_rows[dom_ptr[b]:dom_ptr[b + 1]], ascending"""
        V = C.c_int()
        _check(load().hda_schwarz_domains(self.h, C.byref(V), None, None))
        ptr, rows = np.zeros(V.value + 1, dtype=np.int32), np.zeros(max(self.info()["n_ext"], 1), dtype=np.int32)
        _check(load().hda_schwarz_domains(self.h, C.byref(V), _ip(ptr), _ip(rows)))
        return ptr, rows[:ptr[-1]]

    def factors(self):
        """Block-diagonal factors of all subdomains in the extended numbering (strict lower part L with unit diagonal, rest U)."""
        return _new_csr(load().hda_ilu_factors, self.h, -1, owned=False, keep=self)

    def apply(self, r):
        """One application from a zero guess (max_iter iterations x += M^-1 (r - A x))."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(load().hda_amg_vcycle(self.h, _dp(r), _dp(z)))
        return z


def _fsai_info(h, level):
    v, d = (C.c_int64 * 9)(), (C.c_double * 6)()
    _check(load().hda_fsai_info(h, level, v, d))
    return dict(n=v[0], nnz_factor=v[1], fallback_rows=v[2], blocks=v[3], class_rows={4: v[4], 8: v[5], 16: v[6], 32: v[7], 64: v[8]},
                omega=d[0], apply_bytes=d[1], setup_ms=dict(pattern=d[2], local=d[3], transpose=d[4], omega=d[5]))


class Fsai:
    """'preconditioner: fsai' with algo_type bj-sfsai: the static factorised sparse approximate inverse
    M^-1 = omega G^T G; usable as amg= in pcg()/gmres()/fgmres()/bicgstab()."""

    def __init__(self, A, num_levels=1, threshold=1e-3, max_nnz_row=15, eig_max_iters=5, max_iter=1, blocks=1, block_part=None):
        """blocks: 1 one block, 0 the setup's choice, V the even split unless block_part names the V + 1 row starts"""
        self.A = A
        self.h = C.c_void_p()
        _check(load().hda_fsai_create(A.h, num_levels, threshold, max_nnz_row, eig_max_iters, max_iter, *_blocks_or(blocks, block_part),
                                      C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    def factor(self):
        """G: rows column-sorted, the diagonal last"""
        return _new_csr(load().hda_fsai_factor, self.h, -1, owned=False, keep=self)

    def info(self):
        """dict: n, nnz_factor, fallback_rows, blocks, class_rows (rows per lane class), omega, apply_bytes, setup_ms"""
        return _fsai_info(self.h, -1)

    @property
    def omega(self):
        return self.info()["omega"]

    def apply(self, r):
        """One application from a zero guess (max_iter iterations x += omega G^T G (r - A x))."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(load().hda_amg_vcycle(self.h, _dp(r), _dp(z)))
        return z


class Ams:
    """'preconditioner: ams': the auxiliary-space Maxwell preconditioner for A (n_e x n_e) with the discrete gradient
    G (n_e x n_v, a Csr) and coords = the vertex coordinate vectors; usable as amg= in pcg()/gmres()/fgmres()/bicgstab().
    alpha / beta: AmgParams of the BoomerAMG on Pi^T A Pi / G^T A G (None = Ams.amg_params)."""

    def __init__(self, A, G, coords, dimension=3, cycle_type=1, relax_times=1, relax_weight=1.0, alpha=None, beta=None, max_iter=1):
        self.A, self.G = A, G
        nv = G.ncols
        c = [np.ascontiguousarray(v, dtype=np.float64) for v in coords]
        while len(c) < 3:
            c.append(np.zeros(nv))
        assert all(v.size == nv for v in c), "one coordinate per column of G"
        self.alpha = alpha if alpha is not None else Ams.amg_params(dimension)
        self.beta = beta if beta is not None else Ams.amg_params(1)
        self.h = C.c_void_p()
        _check(load().hda_ams_create(A.h, G.h, _dp(c[0]), _dp(c[1]), _dp(c[2]), dimension, cycle_type, relax_times, relax_weight, max_iter,
                                     C.byref(self.alpha), C.byref(self.beta), C.byref(self.h)))

    @staticmethod
    def amg_params(num_functions=1, **kw):
        """AmgParams of a subspace solver: the reference's GPU-build AMS defaults with the free parameters of DESIGN section 18"""
        p = AmgParams()
        load().hda_ams_default_amg_params(C.byref(p), num_functions)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p

    def __del__(self):
        if getattr(self, "h", None):
            load().hda_amg_destroy(self.h)
            self.h = None

    def _matrix(self, which):
        return _new_csr(load().hda_ams_matrix, self.h, which, owned=False, keep=self)

    def pi(self):
        return self._matrix(0)

    def a_g(self):
        """G^T A G after the zero-row repair"""
        return self._matrix(1)

    def a_pi(self):
        """Pi^T A Pi after the zero-row repair"""
        return self._matrix(2)

    def info(self):
        """dict: n_e, n_v, nnz_pi, nnz_a_g, nnz_a_pi, fixed_rows_g, fixed_rows_pi, levels_g, levels_pi, setup_ms, apply_bytes"""
        v, ms = (C.c_int64 * 8)(), (C.c_double * 5)()
        _check(load().hda_ams_info(self.h, v, ms))
        return dict(n_e=v[0], n_v=v[1], nnz_pi=v[2], nnz_a_g=v[3], nnz_a_pi=v[4], fixed_rows_g=v[5], fixed_rows_pi=v[6],
                    levels_g=v[7] // 256, levels_pi=v[7] % 256,
                    setup_ms=dict(pi=ms[0], products=ms[1], b_g=ms[2], b_pi=ms[3]), apply_bytes=ms[4])

    def apply(self, r):
        """One application from a zero guess (max_iter cycles)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(load().hda_amg_vcycle(self.h, _dp(r), _dp(z)))
        return z


def precond_time(M, reps=20):
    """Average device ms of one application of an Ilu / Schwarz / Ams / Fsai handle (vectors stay on the device)."""
    ms = C.c_double()
    _check(load().hda_precond_time(M.h, reps, C.byref(ms)))
    return ms.value


def _krylov(fn, A, b, amg, kp, x0):
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
    hist = np.zeros(kp.max_iter + 2)
    it, conv, frel = C.c_int(), C.c_int(), C.c_double()
    _check(fn(A.h, amg.h if amg is not None else None, C.byref(kp), _dp(b), _dp(x), _dp(hist),
              C.byref(it), C.byref(conv), C.byref(frel)))
    return dict(x=x, iters=it.value, converged=bool(conv.value), final_rel=frel.value,
                hist=hist[:it.value + 1].copy())


def pcg(A, b, amg=None, kp=None, x0=None):
    return _krylov(load().hda_pcg, A, b, amg, kp or KrylovParams.default(False), x0)


def gmres(A, b, amg=None, kp=None, x0=None):
    return _krylov(load().hda_gmres, A, b, amg, kp or KrylovParams.default(True), x0)


def fgmres(A, b, amg=None, kp=None, x0=None):
    return _krylov(load().hda_fgmres, A, b, amg, kp or KrylovParams.default(True), x0)


def bicgstab(A, b, amg=None, kp=None, x0=None):
    return _krylov(load().hda_bicgstab, A, b, amg, kp or KrylovParams.default(False), x0)


def pcg_multi(A, B, amg=None, kp=None, X0=None):
    """k <= 8 PCG solves in lockstep, one per column of B (n x k; X0: the initial guesses, zero by default).  Returns a list of the
    dicts pcg returns, one per column."""
    kp = kp or KrylovParams.default(False)
    B = _cols(B)
    n, k = B.shape
    bt = np.ascontiguousarray(B.T)
    xt = np.zeros_like(bt) if X0 is None else np.ascontiguousarray(_cols(X0).T).copy()
    hist = np.zeros((max(k, 1), kp.max_iter + 1))
    it, conv, frel = np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1))
    _check(load().hda_pcg_multi(A.h, amg.h if amg is not None else None, C.byref(kp), k, _dp(bt), _dp(xt), _dp(hist), _ip(it), _ip(conv), _dp(frel)))
    return [dict(x=xt[j].copy(), iters=int(it[j]), converged=bool(conv[j]), final_rel=float(frel[j]), hist=hist[j, :it[j] + 1].copy())
            for j in range(k)]


MBLAS_OPS = {"dot": 0, "update": 1, "dir": 2}
SPMM_MODES = {"plain": 0, "resid": 1, "jacobi": 2}


def multi_blas(op, U, V=None, P=None, S=None, alpha=None, beta=None, active=None):
    """The batched BLAS-1 of the PCG recurrences on the k <= 8 columns of n x k arrays (an MBLAS_OPS name).  dot: the k values <U_j,
    V_j>.  update: (U + alpha_j P, V - alpha_j S, the k values <V_j, V_j> afterwards).  dir: P + beta_j U.  A column whose active
    flag is 0 gets alpha_j = beta_j = 0."""
    U = _cols(U)
    n, k = U.shape
    t = lambda v: None if v is None else np.ascontiguousarray(_cols(v).T).copy()
    ut, vt, pt, st = t(U), t(V), t(P), t(S)
    p = lambda v: None if v is None else _dp(v)
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    al, be = f(alpha), f(beta)
    ac = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    out = np.zeros(max(k, 1))
    _check(load().hda_multi_blas(MBLAS_OPS[op], k, n, p(al), p(be), None if ac is None else _ip(ac), p(pt), p(st), p(ut), p(vt), _dp(out)))
    if op == "dot":
        return out[:k].copy()
    if op == "update":
        return ut.T.copy(), vt.T.copy(), out[:k].copy()
    return ut.T.copy()


def time_kernel_multi(kind, A, k, amg=None, reps=20):
    """time_kernel for the batched kernels on k columns: kind 0 product, 1 Jacobi sweep, 2 residual, 3 one batched V-cycle"""
    ms, by = C.c_double(), C.c_double()
    _check(load().hda_time_kernel_multi(kind, A.h, amg.h if amg is not None else None, k, reps, C.byref(ms), C.byref(by)))
    return ms.value, by.value


def time_kernel(kind, A, amg=None, reps=20):
    ms, by = C.c_double(), C.c_double()
    _check(load().hda_time_kernel(kind, A.h, amg.h if amg is not None else None, reps, C.byref(ms), C.byref(by)))
    return ms.value, by.value


def solve_device(A, amg=None, kp=None, b=None, solver=0, nsolves=1, profile_k1=True):
    """nsolves device-resident solves from x0 = 0 against an existing hierarchy."""
    kp = kp or KrylovParams.default(bool(solver))
    times = np.zeros(max(nsolves, 1))
    it = C.c_int()
    d = [C.c_double() for _ in range(4)]
    bb = None if b is None else _dp(np.ascontiguousarray(b, dtype=np.float64))
    _check(load().hda_solve_device(A.h, amg.h if amg is not None else None, C.byref(kp), solver, bb, nsolves,
                                   _dp(times), C.byref(it), C.byref(d[0]), C.byref(d[1]), C.byref(d[2]),
                                   C.byref(d[3]) if profile_k1 else None))
    return dict(solve_ms=times, iters=it.value, final_rel=d[0].value, r0=d[1].value, true_rel=d[2].value,
                k1_avg_ms=d[3].value, precond_calls=load().hda_last_precond_calls())


def pcg_iteration_bytes(A):
    return load().hda_pcg_iteration_bytes(A.h)


def format_bytes(A, amg=None):
    """Bytes really streamed when operators are stencil-coded: dict(pcg_iteration, vcycle, spmv, coded)."""
    a, b, c, d = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    _check(load().hda_format_bytes(A.h, amg.h if amg is not None else None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"pcg_iteration": a.value, "vcycle": b.value, "spmv": c.value, "coded": d.value in (1, 2), "row_coded": d.value == 2,
            "windowed": d.value in (3, 5), "value_coded": d.value in (4, 5)}


# kernel ids of csr_form (HDA_FORM_* of include/hypredrv_amd.h) and product modes of spmv_mode (HDA_SPMV_*)
FORMS = {-1: "none", 0: "lane_group", 1: "stream", 2: "window", 3: "window_runs", 4: "coded", 5: "rowclass"}
SPMV_MODES = {"plain": 0, "plain_dot": 1, "resid": 2, "jacobi": 3, "jacobi_dot": 4, "scaled_copy": 5}


def air_restriction(A, cf, distance=2, strong_th=0.25, filter_th=0.0):
    """Approximate ideal restriction (restriction_type air_1 / air_2) of the square operator A for the splitting cf
    (> 0 C, < 0 F), built on the device.  Returns (R, stats): R a Csr (C points x rows), stats dict(fallback, max_m, small, mid,
    large) -- rows that fell back to injection, the largest neighbourhood, C rows solved by each tier."""
    st = np.zeros(5, dtype=np.int64)
    out = C.c_void_p()
    _check(load().hda_air_restriction(A.h, _marker(cf), int(distance), float(strong_th), float(filter_th), C.byref(out),
                                      st.ctypes.data_as(C.POINTER(C.c_int64))))
    return Csr(out), dict(fallback=int(st[0]), max_m=int(st[1]), small=int(st[2]), mid=int(st[3]), large=int(st[4]))


def csr_form(A, nown=-1):
    """The kernel the product of A runs on: the whole product (nown < 0) or the owned-column half of the split product with nown
    owned columns.  dict(kernel (a FORMS name), lpr, value_coded, escapes, rc_esc_rows, maxrow, blocks (chunks or windows), vc_packed
    (value-coded with packed escapes: the escape slots of its kernel, 512 or 640, else 0))."""
    info = np.zeros(8, dtype=np.int32)
    _check(load().hda_csr_form(A.h, nown, _ip(info)))
    return dict(kernel=FORMS[int(info[0])], lpr=int(info[1]), value_coded=bool(info[2]), escapes=int(info[3]),
                rc_esc_rows=int(info[4]), maxrow=int(info[5]), blocks=int(info[6]), vc_packed=int(info[7]))


def spmv_mode(A, mode, x, nown=-1, alpha=1.0, beta=0.0, yin=None, in_place=False, b=None, dinv=None, w=None, dinv2=None, y2=None):
    """One product of the family (a SPMV_MODES name) through the entry the solver uses; nown >= 0: the split product.  in_place:
    yin is passed as y itself (y starts as yin).  y2: what the scaled copy starts from (rows it leaves alone come back unchanged).
    Returns dict(y, y2, dot, epilogue_taken)."""
    n = A.nrows
    f64 = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    x, yin, b, dinv, w, dinv2 = f64(x), f64(yin), f64(b), f64(dinv), f64(w), f64(dinv2)
    y = yin.copy() if in_place else np.zeros(n)
    y2 = (np.zeros(n) if y2 is None else f64(y2).copy()) if dinv2 is not None else None
    p = lambda v: None if v is None else _dp(v)
    dot, taken = C.c_double(), C.c_int()
    _check(load().hda_spmv_mode(A.h, SPMV_MODES[mode], nown, alpha, beta, p(x), _dp(y) if in_place else p(yin), p(b), p(dinv), p(w),
                                p(dinv2), _dp(y), p(y2), C.byref(dot), C.byref(taken)))
    return dict(y=y, y2=y2, dot=dot.value, epilogue_taken=bool(taken.value))


def probe_spmv(A, mode):
    """Arm the launch-timing probe on matrix A (None disarms); mode 0 y=Ax, 1 residual, 2 Jacobi sweep."""
    _check(load().hda_probe_spmv(A.h if A is not None else None, mode))


def probe_read():
    ms, n = C.c_double(), C.c_int()
    _check(load().hda_probe_read(C.byref(ms), C.byref(n)))
    return ms.value, n.value


def probe_add(A, mode):
    """Arm one more probe (several may be armed at once); returns its id for probe_read_id."""
    k = C.c_int()
    _check(load().hda_probe_add(A.h, mode, C.byref(k)))
    return k.value


def probe_read_id(k):
    ms, n = C.c_double(), C.c_int()
    _check(load().hda_probe_read_id(k, C.byref(ms), C.byref(n)))
    return ms.value, n.value


def borrow(hypredrv_obj):
    """(Csr, Amg) views of what a hypredrv.Hypredrv object built (level-0 operator + hierarchy); borrowed, not copied."""
    a, g = C.c_void_p(), C.c_void_p()
    _check(load().hda_borrow_hypredrv(hypredrv_obj.h, C.byref(a), C.byref(g)))
    A = Csr(a, owned=True, keep=hypredrv_obj)  # destroying the view does not touch the operator
    amg = Amg.__new__(Amg)
    amg.A, amg.params, amg.h = A, None, g
    return A, amg


def borrow_matrix(hypredrv_obj):
    """Csr view of the level-0 operator of a hypredrv.Hypredrv object whatever its preconditioner is (MGR, ILU, ...)."""
    a = C.c_void_p()
    _check(load().hda_borrow_hypredrv(hypredrv_obj.h, C.byref(a), None))
    return Csr(a, owned=True, keep=hypredrv_obj)


class DeviceBuffer:
    """A raw HBM buffer from the library's allocator (hda_dev_alloc): what a caller without torch hands to the IJ calls of an object
    initialised with HYPRE_MEMORY_DEVICE.  .ptr is the device address, .nbytes its size; dtype and shape only describe the content."""

    def __init__(self, nbytes, dtype=np.uint8, shape=None):
        self.nbytes = int(nbytes)
        self.dtype = np.dtype(dtype)
        self.shape = (self.nbytes // self.dtype.itemsize,) if shape is None else tuple(shape)
        p = C.c_void_p()
        _check(load().hda_dev_alloc(self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    @staticmethod
    def from_numpy(a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        b = DeviceBuffer(a.nbytes, a.dtype, a.shape)
        _check(load().hda_dev_upload(b.ptr, a.ctypes.data, a.nbytes))
        return b

    @staticmethod
    def empty(n, dtype=np.float64):
        return DeviceBuffer(int(n) * np.dtype(dtype).itemsize, dtype, (int(n),))

    def to_numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        _check(load().hda_dev_download(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def __len__(self):
        return self.shape[0] if self.shape else 0

    def __del__(self):
        if getattr(self, "ptr", 0):
            load().hda_dev_free(self.ptr)
            self.ptr = 0


def device_pointer(a):
    """The device address behind a DeviceBuffer, an object with __cuda_array_interface__ (a torch tensor on the GPU) or data_ptr(); None
    stays None (the NULL index array of the IJ vector calls)."""
    if a is None:
        return None
    if isinstance(a, DeviceBuffer):
        return a.ptr
    if hasattr(a, "__cuda_array_interface__"):
        return int(a.__cuda_array_interface__["data"][0])
    if hasattr(a, "data_ptr"):
        return int(a.data_ptr())
    raise TypeError(f"not a device array: {type(a).__name__} (DeviceBuffer, __cuda_array_interface__ or data_ptr() expected)")


def download_device(ptr, n, dtype=np.float64):
    """n elements behind a raw device address as a numpy array"""
    out = np.empty(int(n), dtype=dtype)
    _check(load().hda_dev_download(out.ctypes.data, ptr, out.nbytes))
    return out


def borrow_ij(handle):
    """Csr view of the operator behind an assembled HYPRE_IJMatrix handle (hypredrv.ij_matrix / ij_matrix_assemble): columns >= the
    local column count are ghosts.  .ghost_gids: their ascending global ids.  Borrowed: keep the handle alive."""
    A = _new_csr(load().hda_borrow_ij_matrix, handle, owned=True, keep=handle)  # destroying the view does not touch the operator
    n = C.c_int()
    _check(load().hda_ij_ghost_gids(handle, None, 0, C.byref(n)))
    g = np.zeros(max(n.value, 1), dtype=np.int64)
    _check(load().hda_ij_ghost_gids(handle, g.ctypes.data_as(C.POINTER(C.c_longlong)), n.value, C.byref(n)))
    A.ghost_gids = g[:n.value]
    return A


IJ_PATHS = ("none", "csr", "sort")


def ij_last_assembly():
    """The last device-side HYPRE_IJMatrixAssemble of this rank: dict(path ("none", "csr": the stacked calls were a CSR block, "sort":
    sort + run reduction), stacked, merged, sort_ms, reduce_ms)"""
    v = (C.c_double * 5)()
    _check(load().hda_ij_last_assembly(v))
    return dict(path=IJ_PATHS[int(v[0])], stacked=int(v[1]), merged=int(v[2]), sort_ms=v[3], reduce_ms=v[4])


def comm_stats(reset=False):
    v = (C.c_double * 5)()
    load().hda_comm_stats(v, 1 if reset else 0)
    return dict(allreduce=v[0], exchange=v[1], allreduce_doubles=v[2], exchange_doubles=v[3], overlapped=v[4])


def thread_ranks_lap7(nranks, n, P, yaml, nsolves=1, want_x=False):
    """`nranks` ranks of a row partition as threads of this process (hda_thread_ranks.hip; test seam): AMG-Krylov on the
    generator's 7-pt Laplacian, global grid n, rank grid P.  Returns the dict of one rank-0 result (+ "x" in block numbering)."""
    L = load_testranks()
    out = (C.c_double * 16)()
    err = C.create_string_buffer(4096)
    N = int(n[0]) * int(n[1]) * int(n[2])
    x = np.zeros(N) if want_x else None
    L.hda_thread_ranks_lap7.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.c_char_p, C.c_int]
    rc = L.hda_thread_ranks_lap7(int(nranks), (C.c_int * 3)(*n), (C.c_int * 3)(*P), yaml.encode(), int(nsolves), out,
                                 x.ctypes.data_as(C.POINTER(C.c_double)) if want_x else None, err, len(err))
    if rc != 0:
        raise LibraryError(f"hda_thread_ranks_lap7 failed ({rc}): {err.value.decode()}")
    keys = ("iters", "converged", "final_rel", "norm", "l1", "linf", "allreduce", "exchange", "overlapped", "allreduce_doubles",
            "exchange_doubles", "vcycles", "partitioned_levels", "iters_spread", "world")
    res = {k: out[i] for i, k in enumerate(keys)}
    for k in ("iters", "vcycles", "partitioned_levels", "iters_spread", "world"):
        res[k] = int(res[k])
    res["converged"] = bool(res["converged"])
    if want_x:
        res["x"] = x
    return res


def run_thread_ranks(nranks, body):
    """Test seam: `nranks` Python threads, each joined to one in-process world as its rank (hda_thread_world_*), run
    body(rank, nranks) -- which drives the public API like one rank of an MPI job would -- and return the list of results in rank
    order.  ctypes releases the interpreter lock inside library calls, so ranks blocked in a collective do not stall the others.
    A rank that raises releases its peers with an error; the first exception is re-raised here."""
    import threading
    L = load_testranks()
    L.hda_thread_world_create.restype = C.c_void_p
    L.hda_thread_world_join.argtypes = [C.c_void_p, C.c_int]
    L.hda_thread_world_leave.argtypes = [C.c_void_p, C.c_int]
    L.hda_thread_world_destroy.argtypes = [C.c_void_p]
    L.hda_thread_world_destroy.restype = None
    world = L.hda_thread_world_create(int(nranks))
    if not world:
        raise LibraryError("hda_thread_world_create failed")
    res, errs = [None] * nranks, [None] * nranks

    def run(rank):
        failed = 0
        try:
            if L.hda_thread_world_join(world, rank) != 0:
                raise LibraryError(f"rank {rank} could not join the thread world")
            res[rank] = body(rank, nranks)
        except BaseException as e:  # noqa: BLE001 - reported by the caller's thread below
            errs[rank], failed = e, 1
        finally:
            L.hda_thread_world_leave(world, failed)

    th = [threading.Thread(target=run, args=(r,), name=f"hda-rank-{r}") for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    L.hda_thread_world_destroy(world)
    first = [e for e in errs if e is not None and "another rank failed" not in str(e)] or [e for e in errs if e is not None]
    if first:
        raise first[0]
    return res


def comm_name():
    return load().hda_comm_name().decode()


def check_row_total(nrows, row_len):
    """Run the int32 size guard of the setup stages on nrows rows of row_len entries (raises LibraryError past 2^31-1)."""
    _check(load().hda_check_row_total(int(nrows), int(row_len)))


def memory_stats():
    a, b = C.c_double(), C.c_double()
    load().hda_memory_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def memory_cached():
    return load().hda_memory_cached()


def memory_driver_stats(reset=False):
    """hipMalloc calls that reached the driver since the last reset, host ms spent in them, bytes they returned."""
    v = (C.c_double * 3)()
    load().hda_memory_driver_stats(v, 1 if reset else 0)
    return {"hipmalloc_calls": int(v[0]), "hipmalloc_ms": v[1], "hipmalloc_gb": v[2] / 1e9}


def memory_trim():
    """cached device blocks of this thread's allocator back to the driver (another process is about to need the memory)"""
    _check(load().hda_memory_trim())


def measure_rnd(n, seed=2747, level=0, row_offset=0):
    """The random part in [0, 1) of the coarsening measures of n rows (the stream of PMIS, HMIS, CLJP and Falgout)."""
    out = np.zeros(max(n, 0))  # (a negative n is the library's to refuse)
    _check(load().hda_measure_rnd(n, seed, level, row_offset, _dp(out)))
    return out


def sync():
    _check(load().hda_device_sync())
