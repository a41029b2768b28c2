"""CPU tests that pin tests/coarsen_reference.py, the yardstick of the cljp / rs / falgout coarsenings: hand-worked
cases (the expected vectors below were worked out on paper from the definitions in the module's docstring, bucket by bucket and edge by
edge; none was produced by running code), the oracle's Ruge first pass and measure stream, and the invariants the reference satisfies
on the inputs of the device tests -- tests/test_gpu_coarsen_family.py asserts exactly those on the device."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarsen_reference as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graph(n, S):
    """(A, smask) whose strong entries are exactly S (row -> columns it depends on); diagonal 4, strong entries -1."""
    rows, cols, v = [], [], []
    for i in range(n):
        for j in sorted(set(S.get(i, [])) | {i}):
            rows.append(i)
            cols.append(j)
            v.append(4.0 if i == j else -1.0)
    A = sp.csr_matrix((v, (rows, cols)), shape=(n, n))
    A.sort_indices()
    sm = (A.indices != np.repeat(np.arange(n), np.diff(A.indptr))).astype(np.uint8)
    return A, sm


def lap1(n):
    return {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)}


def test_lap1d_by_hand():
    """Seven points, measures 1 2 2 2 2 2 1.  rs: point 1 heads the bucket of measure 2, its neighbour 2 turns F and lifts 3 to measure
    3, and so on: F C F C F C F, nothing for the second pass.  cljp with the random parts below: round 1 D = {2, 4} (2.9 and 2.8 top
    their neighbours), which leaves w = 1 1 . 0 . 1 1 and the live pairs 0 - 1 and 5 - 6; round 2 turns 3 F and D = {1, 6}; then 0 and
    5 have lost their last dependant."""
    A, sm = graph(7, lap1(7))
    assert np.array_equal(cr.rs_blocks(A, sm), [-1, 1, -1, 1, -1, 1, -1])
    st = {}
    assert np.array_equal(cr.cljp(A, sm, [0.1, 0.2, 0.9, 0.3, 0.8, 0.4, 0.5], st), [-1, 1, 1, -1, 1, -1, 1])
    assert st["rounds"] == 2
    # the true operator and mask give the same graph
    L = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(7, 7)).tocsr()
    assert np.array_equal(cr.strength(L, 0.25), sm)


def test_lap2d_3x3_rs_by_hand():
    """5-point Laplacian on 3 x 3 (i = x + 3 y), measures 2 3 2 3 4 3 2 3 2.  The centre 4 is the first C point; its neighbours 1, 3, 5,
    7 turn F in that order and lift the corners: 0 to 4 (through 1 and 3), 2 to 4 (1, 5), 6 to 4 (3, 7), 8 to 4 (5, 7), listed 0 2 6 8
    in the bucket of measure 4; they become C one after the other.  Every F point's neighbours are C: the second pass has no work."""
    g = {}
    for y in range(3):
        for x in range(3):
            g[x + 3 * y] = [(x + dx) + 3 * (y + dy) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)) if 0 <= x + dx < 3 and 0 <= y + dy < 3]
    A, sm = graph(9, g)
    want = [1, -1, 1, -1, 1, -1, 1, -1, 1]
    assert np.array_equal(cr.rs_blocks(A, sm), want)
    assert np.array_equal(cr.rs_blocks(A, sm, second_pass=False), want)
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(3, 3))
    L = (sp.kron(sp.identity(3), T) + sp.kron(T, sp.identity(3))).tocsr()
    L.eliminate_zeros()
    L.sort_indices()
    assert np.array_equal(cr.strength(L, 0.25), sm) and np.array_equal(cr.rs_blocks(L, sm), want)


def test_second_pass_fires_both_branches():
    """Two components.  A ring of five (rows 0-4): the first pass gives C F C F F, the F pair 3 -> 4 shares no C point (3 depends on 2,
    4 on 0), so the visit of 3 makes 4 a tentative C point, and it stays.  Twelve rows 5-16: three hubs 5, 6, 7 (each with two leaves
    and one of 8, 9, 10 depending on them) become C; 8 depends on 5, 9 and 10; 9 depends on 6 only, 10 on 7 only.  The visit of 8 finds
    9 without a common C point (tentative), then 10 as well: 8 itself becomes C and 9 goes back to F."""
    ring = {i: [(i - 1) % 5, (i + 1) % 5] for i in range(5)}
    hubs = {0: [3], 1: [4], 2: [5], 3: [0, 4, 5], 4: [1], 5: [2], 6: [0], 7: [0], 8: [1], 9: [1], 10: [2], 11: [2]}
    both = dict(ring)
    both.update({5 + i: [5 + j for j in v] for i, v in hubs.items()})
    A, sm = graph(17, both)
    assert np.array_equal(cr.rs_blocks(A, sm, second_pass=False), [1, -1, 1, -1, -1] + [1, 1, 1, -1, -1, -1] + [-1] * 6)
    log = []
    assert np.array_equal(cr.rs_blocks(A, sm, log=log), [1, -1, 1, -1, 1] + [1, 1, 1, 1, -1, -1] + [-1] * 6)
    assert log == [("tentative", 3, 4), ("promoted", 8)]
    assert cr.ff_pairs_without_common_c(A, sm, cr.rs_blocks(A, sm, second_pass=False)) == [(3, 4), (4, 3), (8, 9), (8, 10)]


def test_isolated_row():
    """A 1-D Laplacian of five points and a sixth row with its diagonal only: special F (-3) in all three coarsenings.  cljp: D = {2},
    then {0, 4}, then 1 and 3 have no dependant left.  falgout on one block keeps the C points 1 and 3 of rs; their step 3 takes every
    dependant from 0, 2 and 4, which become F."""
    A, sm = graph(6, lap1(5))
    rnd = [0.5, 0.1, 0.7, 0.2, 0.6, 0.9]
    assert np.array_equal(cr.rs_blocks(A, sm), [-1, 1, -1, 1, -1, -3])
    assert np.array_equal(cr.cljp(A, sm, rnd), [1, -1, 1, -1, 1, -3])
    assert np.array_equal(cr.falgout_blocks(A, sm, [0, 6], rnd), [-1, 1, -1, 1, -1, -3])
    # blocks 0-2 | 3-5: the chain 0 - 1 - 2 gives F C F; in the second block 3 and 4 depend on each other only (measures 1 1): 3 is C
    assert np.array_equal(cr.rs_blocks(A, sm, [0, 3, 6]), [-1, 1, -1, 1, -1, -3])


def test_first_pass_strength_and_stream_match_the_oracle(orc):
    """The numpy first pass is the oracle's Ruge first pass (HMIS on one block), the numpy mask the oracle's, and rnd_stream the measure
    stream of PMIS (the oracle's PMIS with these values as its weights is its PMIS from seed and level)."""
    for name, (A, th) in cr.cases(ROOT).items():
        Ao = orc.Csr.from_scipy(A)
        sm = cr.strength(A, th)
        n = A.shape[0]
        assert np.array_equal(sm, orc.strength(Ao, th)), name
        assert np.array_equal(cr.rs_blocks(A, sm, second_pass=False), orc.hmis_blocks(Ao, sm, [0, n])), name
        for seed, level in ((2747, 0), (99, 3)):
            assert np.array_equal(orc.pmis(Ao, sm, seed, level), orc.pmis_weights(Ao, sm, cr.rnd_stream(n, seed, level))), name


# the invariants the device is held to (tests/test_gpu_coarsen_family.py): shown here for the reference on the same inputs
def check_invariants(kind, A, sm, cf, part):
    assert cr.all_decided(cf)
    if kind == "rs":  # by construction: inside a block every F -> F pair shares a C point of the block
        assert cr.ff_pairs_without_common_c(A, sm, cf, part) == []
    else:  # cljp, falgout: the same over the whole matrix, and every F point depends on a C point
        assert cr.ff_pairs_without_common_c(A, sm, cf) == []
        assert cr.f_points_without_c(A, sm, cf) == []


def test_reference_invariants_on_the_device_test_inputs():
    for name, (A, th) in cr.cases(ROOT).items():
        sm = cr.strength(A, th)
        n = A.shape[0]
        for seed in cr.SEEDS:
            rnd = cr.rnd_stream(n, seed)
            check_invariants("cljp", A, sm, cr.cljp(A, sm, rnd), None)
            for V in cr.BLOCKS:
                check_invariants("falgout", A, sm, cr.falgout_blocks(A, sm, cr.even_part(n, V), rnd), None)
        for V in cr.BLOCKS:
            part = cr.even_part(n, V)
            check_invariants("rs", A, sm, cr.rs_blocks(A, sm, part), part)


def test_falgout_on_one_block_keeps_every_c_point_of_rs():
    A, th = cr.cases(ROOT)["lap7 6^3"]
    sm = cr.strength(A, th)
    rs = cr.rs_blocks(A, sm)
    fg = cr.falgout_blocks(A, sm, None, cr.rnd_stream(A.shape[0], 2747))
    assert np.all(fg[rs == 1] == 1)
