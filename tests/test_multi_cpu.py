"""What the batched solve promises without a device: its entry points are declared, exported and bound, and
HYPREDRV_AMD_LinearSolverApplyMulti refuses bad arguments and configurations it does not build -- with non-zero error bits and a
message that names the offending key or argument -- before anything touches a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SEAM = ["hda_spmm", "hda_multi_blas", "hda_amg_vcycle_multi", "hda_pcg_multi", "hda_time_kernel_multi"]
PUBLIC = "HYPREDRV_AMD_LinearSolverApplyMulti"


@pytest.fixture(scope="module")
def hd():
    from hypredrive_amd import hypredrv
    hypredrv.lib()
    return hypredrv


def test_seam_names_are_declared_bound_and_exported():
    from hypredrive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hypredrv_amd.h")).read()
    L = _lib.load()
    for name in NEW_SEAM:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None
    import hypredrive_amd as h
    for name in ("pcg_multi", "multi_blas", "time_kernel_multi"):
        assert callable(getattr(h, name))
    assert callable(h.Csr.spmm) and callable(h.Amg.vcycle_multi)


def test_public_entry_is_declared_and_exported(hd):
    header = open(os.path.join(ROOT, "include", "HYPREDRV.h")).read()
    m = re.search(r"HYPREDRV_EXPORT_SYMBOL uint32_t %s\(([^;]*)\);" % PUBLIC, header)
    assert m, "not declared"
    args = " ".join(m.group(1).split())
    assert args == ("HYPREDRV_t hypredrv, int k, HYPRE_MemoryLocation location, const double *b, double *x, HYPRE_BigInt ld, "
                    "int *iters, double *final_rel"), args
    assert getattr(hd.lib(), PUBLIC).argtypes is not None
    assert callable(hd.Hypredrv.solve_multi)


def refused(hd, h, *args):
    with pytest.raises(hd.HypredrvError) as e:
        h.apply_multi(*args)
    assert e.value.code != 0
    return e.value.code, str(e.value)


def test_argument_refusals_need_no_device(hd):
    h = hd.Hypredrv("solver: pcg\npreconditioner: amg\n")
    b, x = np.zeros(16), np.zeros(16)
    bp, xp = b.ctypes.data, x.ctypes.data
    for k in (0, 9, -1):
        code, msg = refused(hd, h, k, bp, xp, 8)
        assert code & hd.ERROR_INVALID_VAL and "k = %d" % k in msg, msg
    code, msg = refused(hd, h, 2, None, xp, 8)
    assert code & hd.ERROR_INVALID_VAL and "b is NULL" in msg, msg
    code, msg = refused(hd, h, 2, bp, None, 8)
    assert code & hd.ERROR_INVALID_VAL and "x is NULL" in msg, msg
    for ld in (0, -3):   # smaller than any local row count
        code, msg = refused(hd, h, 2, bp, xp, ld)
        assert code & hd.ERROR_INVALID_VAL and "ld = %d" % ld in msg, msg
    # every refusal leaves the sticky state as the other calls of the boundary do: described, then cleared by the caller
    assert hd.lib().HYPREDRV_AMD_LastErrorMessage() == b""
    h.close()


@pytest.mark.parametrize("yaml,bit,needle", [
    ("solver: gmres\npreconditioner: amg\n", "ERROR_INVALID_SOLVER", "solver: gmres"),
    ("solver: fgmres\npreconditioner: amg\n", "ERROR_INVALID_SOLVER", "solver: fgmres"),
    ("solver: bicgstab\npreconditioner: amg\n", "ERROR_INVALID_SOLVER", "solver: bicgstab"),
    ("solver: pcg\npreconditioner: ilu\n", "ERROR_INVALID_PRECON", "preconditioner: ilu"),
    ("solver:\n  pcg:\n    max_iter: 50\n  scaling:\n    enabled: on\n    type: rhs_l2\npreconditioner: amg\n", "ERROR_INVALID_VAL", "solver.scaling"),
])
def test_configurations_without_a_batched_form_are_refused_by_key(hd, yaml, bit, needle):
    h = hd.Hypredrv(yaml)
    b, x = np.zeros(16), np.zeros(16)
    code, msg = refused(hd, h, 2, b.ctypes.data, x.ctypes.data, 8)
    assert code & getattr(hd, bit) and needle in msg, msg
    h.close()


def test_no_prior_setup_is_refused(hd):
    h = hd.Hypredrv("solver: pcg\npreconditioner: amg\n")
    b, x = np.zeros(16), np.zeros(16)
    code, msg = refused(hd, h, 2, b.ctypes.data, x.ctypes.data, 8)
    assert code & hd.ERROR_INVALID_SOLVER and "LinearSolverSetup" in msg, msg
    h.close()
