"""HYPREDRV_AMD_LinearSolverApplyMulti (Hypredrv.solve_multi) on the GPU: k right-hand sides against what HYPREDRV_LinearSolverSetup
prepared, compared with k ordinary HYPREDRV_LinearSolverApply calls on the same object; host and device pointers; and the refusals
that need a set-up object to be reached."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

YAML = "solver:\n  pcg:\n    relative_tol: 1.0e-8\npreconditioner: amg\n"
GRID = (12, 12, 12)
N = 12 ** 3


@pytest.fixture(scope="module")
def hd():
    from hypredrive_amd import hypredrv
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return hypredrv


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def set_up(hd, yaml):
    h = hd.Hypredrv(yaml)
    h.set_laplacian7(GRID)
    h.finish_system()
    h.create_and_setup()
    return h


def right_hand_sides():
    rng = np.random.default_rng(5)
    t = np.arange(N) / N
    return np.stack([np.sin(2.0 * np.pi * t), rng.standard_normal(N), np.ones(N), rng.standard_normal(N) * (1.0 + 10.0 * t)], axis=1)


def test_four_right_hand_sides_match_four_applies(hd):
    from hypredrive_amd._lib import DeviceBuffer
    h = set_up(hd, YAML)
    first = h.apply()                      # the system's own right-hand side, before anything batched
    x_first = h.solution()
    B = right_hand_sides()
    ld = N + 3
    X, iters, frel = h.solve_multi(B, ld=ld)
    assert X.shape == (N, 4) and iters.shape == (4,) and frel.shape == (4,)
    # the same through device pointers: the bits of the host call
    bt, xt = np.zeros((4, ld)), np.zeros((4, ld))
    bt[:, :N] = B.T
    Bd, Xd = DeviceBuffer.from_numpy(bt.ravel()), DeviceBuffer.from_numpy(xt.ravel())
    _, iters_d, frel_d = h.solve_multi(Bd, X0=Xd, device=True, ld=ld)
    Xdev = Xd.to_numpy().reshape(4, ld)
    assert np.array_equal(bits(Xdev[:, :N].T), bits(X)) and not Xdev[:, N:].any()   # (the gap between two vectors is not written)
    assert np.array_equal(iters_d, iters) and np.array_equal(bits(frel_d), bits(frel))
    # an ordinary apply afterwards returns what it returned before: the system's vectors and the solver were not touched
    again = h.apply()
    assert again["iters"] == first["iters"] and again["converged"] == first["converged"]
    assert np.array_equal(bits(h.solution()), bits(x_first)) and bits([again["final_rel"]])[0] == bits([first["final_rel"]])[0]
    # four applies with the same right-hand sides
    for j in range(4):
        h.set_rhs_array(0, N - 1, B[:, j])
        r = h.apply()
        x = h.solution()
        assert r["converged"] and iters[j] == r["iters"], (j, iters[j], r["iters"])
        assert np.linalg.norm(X[:, j] - x) / np.linalg.norm(x) < 1e-10, j
        assert abs(frel[j] - r["final_rel"]) <= 1e-8 * r["final_rel"], (j, frel[j], r["final_rel"])
    h.close()


def test_initial_guesses_and_one_column(hd):
    h = set_up(hd, YAML)
    B = right_hand_sides()[:, :2]
    X, iters, _ = h.solve_multi(B)
    X2, iters2, _ = h.solve_multi(B, X0=X)          # started at the solution: fewer steps, the same answer
    assert np.all(iters2 < iters) and np.linalg.norm(X2 - X) / np.linalg.norm(X) < 1e-7
    X1, it1, _ = h.solve_multi(B[:, 1])             # k = 1 runs the batched code at width 2
    assert it1[0] == iters[1] and np.array_equal(bits(X1[:, 0]), bits(X[:, 1]))
    h.close()


@pytest.mark.parametrize("yaml,bit,needle", [
    ("solver: gmres\npreconditioner: amg\n", "ERROR_INVALID_SOLVER", "solver: gmres"),
    ("solver: pcg\npreconditioner: ilu\n", "ERROR_INVALID_PRECON", "preconditioner: ilu"),
    ("solver: pcg\npreconditioner:\n  amg:\n    relaxation:\n      down_type: 13\n      up_type: 14\n", "ERROR_INVALID_PRECON", "relaxation.down_type 13"),
    ("solver:\n  pcg:\n    max_iter: 50\n  scaling:\n    enabled: on\n    type: rhs_l2\npreconditioner: amg\n", "ERROR_INVALID_VAL", "solver.scaling"),
])
def test_refused_by_name_on_a_set_up_object(hd, yaml, bit, needle):
    h = set_up(hd, yaml)
    before = h.apply()
    with pytest.raises(hd.HypredrvError) as e:
        h.solve_multi(right_hand_sides())
    assert e.value.code & getattr(hd, bit) and needle in str(e.value), str(e.value)
    after = h.apply()                              # the refusal changed nothing
    assert after["iters"] == before["iters"]
    h.close()


def test_ld_smaller_than_n_is_refused(hd):
    h = set_up(hd, YAML)
    b, x = np.zeros(2 * N), np.zeros(2 * N)
    with pytest.raises(hd.HypredrvError) as e:
        h.apply_multi(2, b.ctypes.data, x.ctypes.data, N - 1)
    assert e.value.code & hd.ERROR_INVALID_VAL and "ld = %d" % (N - 1) in str(e.value)
    h.close()
