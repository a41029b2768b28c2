"""The batched V-cycle (Amg.vcycle_multi, Amg::apply_multi of hda_multi.hip) against the single-vector cycle of the same hierarchy.

The reference is Amg.vcycle on each column: the path every other test pins to the oracle.  The bar is the project's V-cycle bar
(DESIGN section 3): relative 2-norm <= 1e-12 per column.  The batched cycle sums every row in its own order (lanes from the row's
length, plain CSR arrays), so it is not bit-equal to the single cycle; it IS bit-equal to itself under a permutation of the columns
and across widths, which is checked through the whole cycle.  What the batched cycle does not run is refused by name at the call,
and a refusal leaves the hierarchy as it was: the single cycle returns the bits it returned before.
"""
import numpy as np
import pytest

from dist_worker import random_mmatrix

pytestmark = pytest.mark.gpu

OPERATORS = ["lap10", "lap16x12x9", "mmatrix"]
PARAMS = {
    "default": {},                                                        # PMIS, ext+i, l1-Jacobi, V(1,1)
    "jacobi0_w08": dict(relax_down=0, relax_up=0, relax_weight=0.8),
    "jacobi7_w08": dict(relax_down=7, relax_up=7, relax_weight=0.8),
    "sweeps_2_1": dict(sweeps_down=2, sweeps_up=1),
}


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


@pytest.fixture(scope="module")
def operators(hd):
    """name -> device operator; built once, never modified"""
    return {"lap10": hd.lap7(10, 10, 10, want_rhs=False), "lap16x12x9": hd.lap7(16, 12, 9, want_rhs=False),
            "mmatrix": hd.Csr.from_scipy(random_mmatrix(3, 1500))}


def rhs(n, k, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    B[:, 0] = np.sin(np.arange(n) * 0.05)   # a smooth column beside the random ones
    return B


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against_single(amg, n):
    assert amg.num_levels >= 3, amg.num_levels
    B = rhs(n, 8, 7)
    single = np.stack([amg.vcycle(B[:, j]) for j in range(8)], axis=1)
    for k in (2, 3, 8):
        X = amg.vcycle_multi(B[:, :k])
        assert X.shape == (n, k)
        for j in range(k):
            assert rel(X[:, j], single[:, j]) <= 1e-12, (k, j, rel(X[:, j], single[:, j]))
    return B


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("op", OPERATORS)
def test_batched_cycle_matches_the_single_cycle(hd, operators, op, pname):
    A = operators[op]
    amg = hd.Amg(A, hd.AmgParams.default(**PARAMS[pname]))
    check_against_single(amg, A.nrows)


@pytest.mark.parametrize("sweeps", [(1, 1), (0, 3)])
def test_air_hierarchy(hd, operators, sweeps):
    """air_1: R is not P^T; the batched cycle restricts with whatever the level stores"""
    A = operators["lap10"]
    amg = hd.Amg(A, hd.AmgParams.default(restrict_type=1, restrict_strong_th=0.25, relax_points=0, relax_down=7, relax_up=7,
                                         sweeps_down=sweeps[0], sweeps_up=sweeps[1]))
    R, P = amg.level_matrix(0, 2).to_scipy(), amg.level_matrix(0, 1).to_scipy()
    assert abs(R - P.T).max() > 1e-3, "the restriction of this hierarchy is P^T: not an AIR case"
    check_against_single(amg, A.nrows)


@pytest.mark.parametrize("op", OPERATORS)
def test_columns_do_not_see_each_other_through_the_cycle(hd, operators, op):
    A = operators[op]
    amg = hd.Amg(A)
    B = rhs(A.nrows, 8, 9)
    X8 = amg.vcycle_multi(B)
    perm = [3, 6, 0, 7, 2, 5, 1, 4]
    assert np.array_equal(bits(amg.vcycle_multi(B[:, perm])), bits(X8[:, perm]))
    assert np.array_equal(bits(amg.vcycle_multi(B[:, :3])), bits(X8[:, :3]))
    assert np.array_equal(bits(amg.vcycle_multi(B[:, [5]])[:, 0]), bits(X8[:, 5]))
    assert np.array_equal(bits(amg.vcycle_multi(B)), bits(X8))   # and a second run repeats the first


REFUSED = {
    "gauss-seidel": (dict(relax_down=6, relax_up=6), "Gauss-Seidel"),
    "chebyshev": (dict(relax_down=16, relax_up=16), "Chebyshev"),
    "ilu smoother": (dict(smooth_type=5, smooth_num_levels=1), "ilu"),
    "points air": (dict(relax_points=1, relax_down=7, relax_up=7), "relaxation.points"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_what_is_not_built_is_refused_by_name_and_leaves_the_hierarchy_alone(hd, operators, case):
    kw, name = REFUSED[case]
    A = operators["lap10"]
    amg = hd.Amg(A, hd.AmgParams.default(**kw))   # the setup itself is as before: nothing is refused there
    b = rhs(A.nrows, 1, 3)[:, 0]
    before = amg.vcycle(b)
    with pytest.raises(hd.LibraryError, match=name):
        amg.vcycle_multi(np.stack([b, 2.0 * b], axis=1))
    assert np.array_equal(bits(amg.vcycle(b)), bits(before))


@pytest.mark.parametrize("k", [0, 9])
def test_width_outside_1_to_8_is_refused_by_name(hd, operators, k):
    amg = hd.Amg(operators["lap10"])
    with pytest.raises(hd.LibraryError, match="k:"):
        amg.vcycle_multi(np.ones((1000, k)))
