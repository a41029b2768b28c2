"""Every route of the device sparse product, the transpose and the row sorts, bit for bit against tests/spgemm_reference.py.

spgemm() chooses its kernel from the content of its inputs; every case here is built to reach one choice and asserts
  (a) through hda_spgemm_last_route that the product took the route that route() predicts and the case is there for,
  (b) rowptr and col equal to the reference's,
  (c) the values equal to product_sequential bit for bit (compared as int64, so signed zeros count),
  (d) every entry within gamma(m) sum|terms| of its exact sum (product_bound: the check that does not share the reference's order).
X and Y are uploaded with the entries of every row shuffled; hda_csr_create sorts them.

Routes taken (tests/test_spgemm_reference.py asserts the same table on the CPU): the LDS kernel at capacities 2048 / 4096 / 8192
(256 / 512 / 1024 threads), staged and unstaged expansion; the hash product for an empty input, a row of more than 4096 products and
a chunk of 2^19 rows or more, single pass and row-batched (HDA_SPGEMM_SLOTS, in child processes); the three routes of sort_rows
(insertion, wavefront network with its one-lane fallback beyond 64 entries, segmented radix sort) behind hda_transpose and
hda_csr_create.  The fourth reason for the hash product, product scratch beyond 30 % of the device memory, needs about 7e9 products
and is not reachable in a test.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as hd
    if hd.device_count() < 1:
        pytest.skip("needs a HIP device")
    return hd


def upload(hd, M, seed=3):
    M = sp.csr_matrix(M)
    return hd.Csr.from_arrays(M.shape[0], M.shape[1], *R.shuffled(M, np.random.default_rng(seed)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """inputs, predicted route, sequential product and bound of a case: computed once, never modified"""
    gen, args, intent = R.CASES[name]
    X, Y = gen(*args)
    rt = R.route(X, Y)
    R.check_intent(rt, intent, X)
    return X, Y, rt, R.product_sequential(X, Y), R.product_bound(X, Y)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def check_product(hd, Ch, rt, C, bound):
    got = hd.spgemm_last_route()
    assert got == R.readback(rt), (got, R.readback(rt))                       # (a)
    assert Ch.dims == (C.shape[0], C.shape[1], C.nnz)
    rp, cj, v = Ch.download()
    assert np.array_equal(rp, C.indptr) and np.array_equal(cj, C.indices)     # (b)
    assert np.array_equal(bits(v), bits(C.data))                              # (c)
    assert R.within_bound(v, bound).all()                                     # (d)
    return rp, cj, v


@pytest.mark.parametrize("name", list(R.CASES))
def test_product_route_by_route(hd, name):
    X, Y, rt, C, bound = reference(name)
    Xh, Yh = upload(hd, X), upload(hd, Y, 4)
    if X.shape[0] == 0:
        assert hd.sort_rows_last_route() == "insertion" and upload(hd, X).dims == (0, 5, 0) and hd.sort_rows_last_route() == "none"
    rp, cj, v = check_product(hd, Xh.matmul(Yh), rt, C, bound)
    if name.startswith("cancellation"):                                       # spelled out: +0.0, -0.0, -0.0, exact survivors, +0.0
        row = lambda i: v[rp[i]:rp[i + 1]]
        assert [list(np.signbit(row(i))) for i in (0, 1, 2, 4)] == [[False] * 3, [True] * 3, [True] * 3, [False] * 3]
        assert not np.any(np.concatenate([row(i) for i in (0, 1, 2, 4)])) and list(row(3)) == [1e-20 * 2.5, 1e-20 * 7.0, 1e-20 * 1e-3]
    if name.startswith("wide"):
        # (hda_csr_create accepts ncols = 2^31 - 1, the largest int: no smaller width had to be substituted)
        assert Yh.ncols == R.WIDE and set(cj) == {0, 2 ** 30, 2 ** 31 - 2}


def test_routes_agree_on_untouched_rows(hd):
    """64 x 64 products on the LDS kernel at capacity 8192; one more entry in the long row sends the whole product to the hash path:
    every other row comes back with the same bits"""
    X, Y, rt, C, _ = reference("long row 64x64")
    X2, _, rt2, C2, _ = reference("long row 65x64")
    assert (rt["path"], rt["capacity"], rt2["path"]) == ("esc", 8192, "hash") and (X != X2).nnz == 1
    Yh = upload(hd, Y)
    a = upload(hd, X).matmul(Yh)
    assert hd.spgemm_last_route()["path"] == "esc"
    b = upload(hd, X2).matmul(Yh)
    assert hd.spgemm_last_route()["path"] == "hash"
    (rpa, cja, va), (rpb, cjb, vb) = a.download(), b.download()
    for lo, hi in ((0, 150), (151, 300)):
        assert np.array_equal(np.diff(rpa[lo:hi + 1]), np.diff(rpb[lo:hi + 1]))
        sa, sb = slice(rpa[lo], rpa[hi]), slice(rpb[lo], rpb[hi])
        assert np.array_equal(cja[sa], cjb[sb]) and np.array_equal(bits(va[sa]), bits(vb[sb]))


def test_batched_hash_product(hd, tmp_path):
    """HDA_SPGEMM_SLOTS is read once per process: child processes with the default budget (one batch), 1024 (every row its own batch:
    the long row's table alone is 16 times the budget and still gets built) and 4096.  All three give the sequential reference."""
    X, Y = R.gen_long_row(*R.BATCHED_INPUT)
    C = R.product_sequential(X, Y)
    for slots in (None, 1024, 4096):
        rt = R.route(X, Y, R.DEFAULT_SLOTS if slots is None else slots)
        assert rt["why_hash"] == "row longer than 4096 products" and (rt["batches"] == 1) == (slots is None)
        got, arr = R.batched_child(slots, tmp_path / f"c_{slots}.npz")
        print(slots, got)
        assert got == R.readback(rt), (slots, got)
        assert got["path"] == "hash" and (got["batches"] > 1) == (slots is not None)
        assert np.array_equal(arr["rp"], C.indptr) and np.array_equal(arr["cj"], C.indices)
        assert np.array_equal(bits(arr["v"]), bits(C.data))


def test_galerkin_product(hd):
    """A.rap(P) = P^T (A P) with empty rows in P and one long column; the read-back is the second product's"""
    A, P = R.gen_galerkin()
    AP = R.product_sequential(A, P)
    Pt = sp.csr_matrix(P.T)
    Pt.sort_indices()
    rt = R.route(Pt, AP)
    assert rt["path"] == "esc" and rt["capacity"] >= 4096 and R.route(A, P)["capacity"] == 2048
    assert (np.diff(P.indptr) == 0).sum() > 100
    Ac = upload(hd, A).rap(upload(hd, P, 4))
    check_product(hd, Ac, rt, R.product_sequential(Pt, AP), R.product_bound(Pt, AP))


def test_inner_dimensions_refused(hd):
    rng = np.random.default_rng(0)
    X, Y = R.rows_matrix([2, 0, 3], 6, rng), R.rows_matrix([1] * 5, 4, rng)
    with pytest.raises(hd.LibraryError, match="inner dimensions"):
        upload(hd, X).matmul(upload(hd, Y))


def same_matrix(hd, Mh, T):
    rp, cj, v = Mh.download()
    assert Mh.dims == (T.shape[0], T.shape[1], T.nnz)
    return np.array_equal(rp, T.indptr) and np.array_equal(cj, T.indices) and np.array_equal(bits(v), bits(T.data))


@pytest.mark.parametrize("name", R.SORT_CASES)
def test_transpose_and_create_sort(hd, name):
    """values are moved, not computed: the device transpose of A = T^T and the upload of T with shuffled rows both equal T in all three
    arrays, each on the sort route the average row length of T selects (rows of 65 and 200 entries inside the wave route take its
    one-lane fallback; empty columns of A are empty rows of T)"""
    T, rt = R.gen_sort(name)
    A = sp.csr_matrix(T.T)
    A.sort_indices()
    Ah = upload(hd, A)
    Th = Ah.transpose()
    assert hd.sort_rows_last_route() == rt
    assert same_matrix(hd, Th, T)
    created = upload(hd, T, 9)
    assert hd.sort_rows_last_route() == rt
    assert same_matrix(hd, created, T)
    assert same_matrix(hd, Ah, A)
