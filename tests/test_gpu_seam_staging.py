"""Staging of the kernel-level seam: every Csr wrapper that hands a strength mask, a C/F marker or row-block starts to the C ABI, on
operators small enough that an off-by-one in a staged length changes the answer or runs off the caller's buffer.

Four operators: no rows at all, one row that is its diagonal, lap7(2, 2, 2) (8 rows, every one a boundary row) and lap7(3, 3, 3)
(27 rows, one interior row).  For every call: output lengths are exactly nrows / nnz; results equal the CPU oracle's bit for bit
wherever the oracle has the routine; a relaxation sweep of every type equals the oracle's to 1e-13 (the bar of the relax tests in
test_gpu_parity.py).  Types 11 / 12 have no oracle routine: their yardstick is the numpy restatement of test_gpu_two_stage_gs.py at
that file's bar, 1e-12 (restated here in a dozen lines).

Vectors handed to the products are small integers and the operators' entries are -1 and 6 (or 1), so every product and every partial
sum is exact in fp64: the order of a wave-parallel reduction cannot show, and bit equality is a fair demand on spmv and matmul as well (the setup arithmetic -- interpolation weights, RAP, l1 norms --
is defined in a fixed order and bit-comparable by design).
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

OPS = ["empty", "diag1", "lap222", "lap333"]
RELAX_TYPES = [0, 3, 4, 6, 7, 8, 11, 12, 13, 14, 18]


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


@pytest.fixture(scope="module")
def ops(hd, orc):
    """name -> (device Csr, oracle Csr, scipy matrix); built once, never modified"""
    out = {}
    for name, M in [("empty", sp.csr_matrix((0, 0))), ("diag1", sp.csr_matrix(np.array([[1.0]])))]:
        out[name] = (hd.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data),
                     orc.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data), M)
    for name, g in [("lap222", (2, 2, 2)), ("lap333", (3, 3, 3))]:
        Ao = orc.lap7(*g)[0]
        out[name] = (hd.lap7(*g, want_rhs=False), Ao, Ao.to_scipy())
    return out


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def arrays(Mh, nrows, ncols):
    """download with the lengths checked: rowptr nrows + 1, columns and values exactly nnz"""
    n, m, nnz = Mh.dims
    rp, cj, v = Mh.download()
    assert (n, m) == (nrows, ncols), ((n, m), (nrows, ncols))
    assert rp.shape == (n + 1,) and cj.shape == (nnz,) and v.shape == (nnz,) and rp[0] == 0 and rp[-1] == nnz
    assert nnz == 0 or (cj.min() >= 0 and cj.max() < max(m, 1))
    return rp, cj, v


def same_as_oracle(Mh, Mo):
    rp, cj, v = arrays(Mh, Mo.nrows, Mo.ncols)
    assert np.array_equal(rp, Mo.rowptr) and np.array_equal(cj, Mo.col) and np.array_equal(bits(v), bits(Mo.val))


def same_as_scipy(Mh, T):
    T = sp.csr_matrix(T)
    T.sort_indices()
    rp, cj, v = arrays(Mh, T.shape[0], T.shape[1])
    assert np.array_equal(rp, T.indptr) and np.array_equal(cj, T.indices) and np.array_equal(bits(v), bits(T.data))


def block_parts(n):
    """the one block, and two ragged blocks where there are rows to split"""
    return [np.array([0, n])] + ([np.array([0, n // 3 + 1, n])] if n >= 2 else [])


def splitting(orc, Ao):
    sm = orc.strength(Ao)
    return sm, orc.pmis(Ao, sm)


@pytest.mark.parametrize("op", OPS)
def test_strength_and_coarsening(hd, orc, ops, op):
    Ah, Ao, M = ops[op]
    n, nnz = M.shape[0], M.nnz
    sm = Ah.strength()
    assert sm.shape == (nnz,) and sm.dtype == np.uint8 and np.array_equal(sm, orc.strength(Ao))
    cf = Ah.pmis(sm)
    assert cf.shape == (n,) and cf.dtype == np.int32 and np.array_equal(cf, orc.pmis(Ao, sm))
    cf = Ah.cljp(sm)
    assert cf.shape == (n,) and cf.dtype == np.int32 and np.all(cf != 0) and Ah.last_rounds >= 0
    for part in block_parts(n):
        cf = Ah.hmis_blocks(sm, part)
        assert cf.shape == (n,) and np.array_equal(cf, orc.hmis_blocks(Ao, sm, part)), list(part)
        for cf in (Ah.rs_blocks(sm, part), Ah.falgout_blocks(sm, part)):
            assert cf.shape == (n,) and cf.dtype == np.int32 and np.all(cf != 0), list(part)
    assert Ah.rs_blocks(sm).shape == (n,) and Ah.falgout_blocks(sm).shape == (n,)  # part=None: the one block


@pytest.mark.parametrize("op", OPS)
def test_interpolation(hd, orc, ops, op):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    sm, cf = splitting(orc, Ao)
    nc = int((cf > 0).sum())
    for name in ("interp_extpi", "interp_mm_extpi", "interp_direct", "interp_standard"):
        for pmax, tf in ((4, 0.0), (2, 0.1)):
            same_as_oracle(getattr(Ah, name)(sm, cf, pmax, tf), getattr(orc, name)(Ao, sm, cf, pmax, tf))
    for P in (Ah.interp_extended(sm, cf), Ah.interp_mm_ext(sm, cf), Ah.interp_one_point(sm, cf)):
        rp, cj, v = arrays(P, n, nc)
        crow = np.flatnonzero(cf > 0)  # a C point interpolates from itself alone, weight 1
        assert np.all(np.diff(rp)[crow] == 1) and np.array_equal(cj[rp[crow]], np.arange(nc)) and np.all(v[rp[crow]] == 1.0)


@pytest.mark.parametrize("op", OPS)
def test_aggressive_stages(hd, orc, ops, op):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    sm, cf1 = splitting(orc, Ao)
    for paths in (1, 2):
        same_as_oracle(Ah.second_strength(sm, cf1, paths), orc.second_strength(Ao, sm, cf1, paths))
    cf2 = Ah.coarsen_second_pass(sm, cf1)
    assert cf2.shape == (n,) and cf2.dtype == np.int32 and np.array_equal(cf2, orc.coarsen_second_pass(Ao, sm, cf1))
    same_as_oracle(Ah.interp_multipass(sm, cf2), orc.interp_multipass(Ao, sm, cf2))
    same_as_oracle(Ah.interp_multipass(sm, cf2).truncate_rows(2, 0.1), orc.truncate_rows(orc.interp_multipass(Ao, sm, cf2), 2, 0.1))
    n1, n2 = int((cf1 > 0).sum()), int((cf2 > 0).sum())
    for plus_i in (False, True):
        P1, P2, P = Ah.interp_agg_two_stage_parts(sm, cf1, cf2, plus_i, 4, 0.0, 4, 0.0)
        a1, a2, a = arrays(P1, n, n1), arrays(P2, n1, n2), arrays(P, n, n2)
        alone = arrays(Ah.interp_agg_second_stage(sm, cf1, cf2, plus_i, 4, 0.0), n1, n2)
        assert all(np.array_equal(x, y) for x, y in zip(a2[:2], alone[:2])) and np.array_equal(bits(a2[2]), bits(alone[2]))
        whole = arrays(Ah.interp_agg_two_stage(sm, cf1, cf2, plus_i, 4, 0.0, 4, 0.0), n, n2)
        assert all(np.array_equal(x, y) for x, y in zip(a[:2], whole[:2])) and np.array_equal(bits(a[2]), bits(whole[2]))


@pytest.mark.parametrize("op", OPS)
def test_products_and_norms(hd, orc, ops, op):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    rng = np.random.default_rng(n)
    x, y = rng.integers(-8, 9, n).astype(np.float64), rng.integers(-8, 9, n).astype(np.float64)
    for got, want in ((Ah.spmv(x), orc.spmv(Ao, x)), (Ah.spmv(x, -1.0, 1.0, y), orc.spmv(Ao, x, -1.0, 1.0, y))):
        assert got.shape == (n,) and np.array_equal(bits(got), bits(want))
    for opt in (1, 4):
        got = Ah.l1_norms(opt)
        assert got.shape == (n,) and np.array_equal(bits(got), bits(orc.l1_norms(Ao, opt)))
        for part in block_parts(n):
            got = Ah.l1_norms_blocks(opt, part)
            assert got.shape == (n,) and np.array_equal(bits(got), bits(orc.l1_norms_blocks(Ao, opt, part))), list(part)
    same_as_scipy(Ah.transpose(), M.T)
    same_as_scipy(Ah.matmul(Ah), M @ M)
    sm, cf = splitting(orc, Ao)
    Po = orc.interp_extpi(Ao, sm, cf, 4, 0.0)
    Ph = Ah.interp_extpi(sm, cf, 4, 0.0)
    same_as_oracle(Ah.rap(Ph), orc.rap(Ao, Po))
    same_as_scipy(Ph.transpose(), Po.to_scipy().T)


@pytest.mark.parametrize("op", OPS)
def test_air_restriction(hd, orc, ops, op):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    _, cf = splitting(orc, Ao)
    nc = int((cf > 0).sum())
    for distance in (1, 2):
        R, st = hd._lib.air_restriction(Ah, cf, distance)
        rp, cj, v = arrays(R, nc, n)
        assert all(c >= 0 for c in st.values()) and st["fallback"] <= nc
        crow = np.flatnonzero(cf > 0)  # row c of R holds the C point's own column with weight 1
        for c, i in enumerate(crow):
            k = np.flatnonzero(cj[rp[c]:rp[c + 1]] == i)
            assert k.size == 1 and v[rp[c] + k[0]] == 1.0, (distance, c)


def two_stage_reference(M, b, x, terms, weight, part=None):
    """u += z_0 + .. + z_terms, z_0 = w D^-1 (b - A u), z_k = -D^-1 L z_{k-1}; L: the strictly lower part inside the row's block"""
    n = M.shape[0]
    C = M.tocoo()
    lo = np.zeros(n, dtype=np.int64) if part is None else part[np.searchsorted(part, np.arange(n), side="right") - 1]
    keep = (C.col < C.row) & (C.col >= lo[C.row])
    L = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=(n, n))
    d = M.diagonal()
    z = weight * (b - M @ x) / d
    x = x + z
    for _ in range(terms):
        z = -(L @ z) / d
        x = x + z
    return x


@pytest.mark.parametrize("rtype", RELAX_TYPES)
@pytest.mark.parametrize("op", OPS)
def test_relax(hd, orc, ops, op, rtype):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    rng = np.random.default_rng(100 * n + rtype)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    got = Ah.relax(b, x0, rtype, 0.9, sweeps=2)
    assert got.shape == (n,)
    want = x0
    for _ in range(2):
        if rtype in (11, 12):
            want = two_stage_reference(M, b, want, rtype - 10, 0.9)
        else:
            want = orc.relax(Ao, orc.l1_norms(Ao, 1 if rtype == 18 else 4), rtype, 0.9, b, want)
    assert rel(got, want) < (1e-12 if rtype in (11, 12) else 1e-13), rel(got, want)


# (hybrid Gauss-Seidel on row blocks of the empty operator is no case here: before the entry staged every vector into at least one element
#  the block sweep refused two empty vectors as "out of place", so there is no earlier behaviour for it to be held to)
@pytest.mark.parametrize("op,rtype", [(op, t) for op in OPS for t in RELAX_TYPES if t not in (0, 7, 18) and (op != "empty" or t in (11, 12))])
def test_relax_blocks(hd, orc, ops, op, rtype):
    Ah, Ao, M = ops[op]
    n = M.shape[0]
    rng = np.random.default_rng(200 * n + rtype)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    for part in block_parts(n):
        got = Ah.relax_blocks(b, x0, part, rtype, 0.9, sweeps=2)
        assert got.shape == (n,)
        want = x0
        for _ in range(2):
            if rtype in (11, 12):
                want = two_stage_reference(M, b, want, rtype - 10, 0.9, part)
            else:
                want = orc.relax_blocks(Ao, orc.l1_norms_blocks(Ao, 4, part), rtype, 0.9, b, want, part)
        assert rel(got, want) < (1e-12 if rtype in (11, 12) else 1e-13), (list(part), rel(got, want))
