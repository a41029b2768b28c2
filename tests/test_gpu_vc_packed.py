"""Packed escapes of a value-coded operator on the list-windowed kernel (k_spmv_win<..., PACK = 512 | 640>; hda_kernels.hip "packed
escapes").

The packed form only changes where the kernel finds an escaped value -- in the chunk's block of escaped values instead of in the CSR
value array -- so every result must equal that of the unpacked form (HDA_VC_PACK=0, read per matrix: both forms live in one process)
BIT FOR BIT, and both lie within the componentwise bound of the exact row-by-row reference (tests/spmv_reference.py, the bound of
tests/test_gpu_spmv_forms.py).  csr_form()["vc_packed"] says which form an operator took: the escape slots of its kernel (512, or 640
= kEscCap when a chunk has more than 512 escapes), or 0 for the unpacked form.

Cases:
  - P0 and R0 of the 7-point Laplacian hierarchy at 72^3 (1.14 M entries each), plain product and the product with the scaled second
    result (EPI);
  - a synthetic operator of 300 000 rows x 4 entries (every chunk is exactly 1024 entries, the last one 896) whose values come from 240
    frequent and 1 060 rare values, with chunks built for the edges: no escape; 100 escapes (numbers past one code range of 15, i.e.
    quotient bits in the position); 128 escapes in the last, partial chunk, its last entry among them; and one chunk with 512 (the most
    the 512-slot kernel takes), 513 (the fewest that need the 640-slot kernel) or 640 = kEscCap escapes;
  - fallbacks to the unpacked form: one chunk with kEscCap + 1 escapes; a chunk of 1025 distinct columns (no spare position bits), beside
    its twin with shared columns that IS packed (chunks of 1025 entries: the kernel's loop past the 1024 prefetched entries); a split
    product through the per-kernel seam, which takes the packed form back; two thread ranks whose overlapped products are split products;
  - a whole AMG-PCG solve at 72^3 with the switch on and off;
  - the byte accounting of a packed operator.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spmv_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_ESC_CAP, CODE_RANGE, CHUNK, LAST_ESC = 640, 15, 1024, 128
N_HIER = 72


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as hd
    if hd.device_count() < 1:
        pytest.skip("needs a HIP device")
    return hd


class pack_switch:
    """HDA_VC_PACK for the operators whose plans are built inside the block (the library reads it per matrix)."""

    def __init__(self, on):
        self.v = "1" if on else "0"

    def __enter__(self):
        self.old = os.environ.get("HDA_VC_PACK")
        os.environ["HDA_VC_PACK"] = self.v

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("HDA_VC_PACK", None)
        else:
            os.environ["HDA_VC_PACK"] = self.old


def both_forms(hd, make):
    """(operator, csr_form) with the switch on and off; the form is asked for inside the switch, which builds the plan."""
    out = {}
    for arm in (True, False):
        with pack_switch(arm):
            M = make()
            out[arm] = (M, hd._lib.csr_form(M))
    return out


def check_products(hd, forms, seed, modes=("plain", "scaled_copy")):
    """Every mode: packed == unpacked bit for bit, and both within the bound of the exact reference (one reference for both)."""
    Mp, Mu = forms[True][0], forms[False][0]
    n, m = Mp.nrows, Mp.ncols
    rng = np.random.default_rng(seed)
    x = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-4, 4, m)
    V = dict(b=rng.standard_normal(n), dinv=rng.uniform(0.1, 2.0, n), w=rng.standard_normal(n), dinv2=rng.uniform(0.5, 2.0, n))
    rp, col, val = Mu.download()
    P = R.Problem(rp, col, val, m, x)
    for mode in modes:
        kw = dict(dinv2=V["dinv2"]) if mode == "scaled_copy" else dict(b=V["b"], dinv=V["dinv"], w=V["w"])
        a = hd._lib.spmv_mode(Mp, mode, x, **kw)
        b = hd._lib.spmv_mode(Mu, mode, x, **kw)
        assert np.all(np.isfinite(a["y"])) and np.any(a["y"] != 0.0)
        assert np.array_equal(a["y"].view(np.int64), b["y"].view(np.int64)), (mode, int(np.sum(a["y"] != b["y"])))
        for r in (a, b):
            err, tol = R.row_errors(P, r["y"], mode, alpha=1.0, beta=0.0, b=V["b"], dinv=V["dinv"])
            bad = np.nonzero(~(err <= tol))[0]
            assert bad.size == 0, (mode, "rows outside the bound", bad[:10], err[bad[:5]], tol[bad[:5]])
        if mode == "scaled_copy":
            assert a["epilogue_taken"] and b["epilogue_taken"]
            assert np.array_equal(a["y2"].view(np.int64), b["y2"].view(np.int64))
            assert np.array_equal((V["dinv2"] * a["y"]).view(np.int64), a["y2"].view(np.int64))
        if mode.endswith("_dot"):
            assert a["dot"] == b["dot"], (mode, a["dot"], b["dot"])
    return P


# ------------------------------------------------------------------ the transfer operators of a hierarchy
@pytest.fixture(scope="module")
def hierarchies(hd):
    out = {}
    for arm in (True, False):
        with pack_switch(arm):
            A = hd.lap7(N_HIER, N_HIER, N_HIER)
            amg = hd.Amg(A)
            ops = {"P": amg.level_matrix(0, 1), "R": amg.level_matrix(0, 2)}
            out[arm] = dict(A=A, amg=amg, ops=ops, forms={k: hd._lib.csr_form(M) for k, M in ops.items()})
    return out


@pytest.mark.parametrize("name", ["P", "R"])
def test_level0_transfer_operator_packed_equals_unpacked(hd, hierarchies, name):
    forms = {arm: (hierarchies[arm]["ops"][name], hierarchies[arm]["forms"][name]) for arm in (True, False)}
    fp, fu = forms[True][1], forms[False][1]
    print(name, forms[True][0].dims, fp, fu)
    assert fp["kernel"] == "window" and fp["value_coded"] and fp["vc_packed"] in (512, 640), fp
    assert fu["kernel"] == "window" and fu["value_coded"] and fu["vc_packed"] == 0, fu
    assert fp["escapes"] == fu["escapes"] and fp["blocks"] == fu["blocks"]  # (escapes: entries outside the 255-entry dictionary, either form)
    check_products(hd, forms, seed=3)


def test_whole_solve_is_the_same_with_and_without_packing(hd, hierarchies):
    res = {}
    for arm in (True, False):
        h = hierarchies[arm]
        res[arm] = hd.pcg(h["A"], h["A"].rhs, h["amg"])
    a, b = res[True], res[False]
    assert a["converged"] and a["iters"] == b["iters"]
    assert np.array_equal(np.asarray(a["hist"]), np.asarray(b["hist"]))
    assert np.array_equal(a["x"], b["x"])
    assert a["final_rel"] == b["final_rel"]


# ------------------------------------------------------------------ synthetic operators
def _alphabet(rng):
    vals = np.unique(rng.choice([-1.0, 1.0], 1400) * 10.0 ** rng.uniform(-3, 3, 1400))[:1300]
    vals = rng.permutation(vals)
    return vals[:240], vals[240:]  # 240 frequent (the dictionary entries that keep their codes), 1 060 rare


def _fill_values(rng, nnz, bounds, special):
    """Frequent values everywhere but for 5 % rare ones; special: {chunk: (number of rare entries, also the chunk's last entry?)}.
    Returns values and the rare mask."""
    freq, rare = _alphabet(rng)
    is_rare = rng.random(nnz) < 0.05
    for c, (cnt, last) in special.items():
        k0, k1 = bounds[c], bounds[c + 1]
        is_rare[k0:k1] = False
        pick = rng.choice(k1 - k0 - (1 if last else 0), cnt - (1 if last else 0), replace=False) + k0
        is_rare[pick] = True
        if last:
            is_rare[k1 - 1] = True
    v = freq[rng.integers(0, freq.size, nnz)]
    v[is_rare] = rare[rng.integers(0, rare.size, int(is_rare.sum()))]
    return v, is_rare


def chunk_bounds(rowptr):
    """First entry of every chunk (+ nnz): chunk c starts at the first row whose first entry is at or past 1024 c (k_wchunk_rows)."""
    nnz = int(rowptr[-1])
    nw = max(1, -(-nnz // CHUNK))
    rows = np.searchsorted(rowptr, np.arange(nw) * CHUNK, side="left")
    return np.concatenate([rowptr[rows], [nnz]]).astype(np.int64)


def gen_edges(seed, cap_chunk_escapes):
    """300 000 rows of 4 entries at columns r + 7 q: chunk c is entries [1024 c, 1024 c + 1024), 1171 whole chunks and one of 896."""
    rng = np.random.default_rng(seed)
    n = 300000
    rowptr = 4 * np.arange(n + 1, dtype=np.int64)
    col = (np.arange(n)[:, None] + 7 * np.arange(4)[None, :]).ravel()
    bounds = chunk_bounds(rowptr)
    last = bounds.size - 2
    assert bounds[last + 1] - bounds[last] == 896 and np.all(np.diff(bounds[:-1]) == CHUNK)
    special = {3: (0, False), 5: (cap_chunk_escapes, False), 7: (100, False), last: (LAST_ESC, True)}
    val, is_rare = _fill_values(rng, rowptr[-1], bounds, special)
    per_chunk = np.add.reduceat(is_rare.astype(np.int64), bounds[:-1])
    return (n, n + 32, rowptr, col, val), per_chunk, bounds


ALL_MODES = ("plain", "scaled_copy", "resid", "jacobi", "plain_dot", "jacobi_dot")


@pytest.mark.parametrize("most,slots,modes", [(512, 512, ALL_MODES), (513, 640, ("plain", "scaled_copy")), (K_ESC_CAP, 640, ALL_MODES)])
def test_synthetic_chunk_edges_packed_equals_unpacked(hd, most, slots, modes):
    csr, per_chunk, bounds = gen_edges(21, most)
    last = per_chunk.size - 1
    assert per_chunk[3] == 0 and per_chunk[5] == most and per_chunk[7] == 100 and per_chunk[last] == LAST_ESC
    assert per_chunk.max() == most and 100 - 1 >= CODE_RANGE  # escape 99 = code 240 + 9, quotient 6
    forms = both_forms(hd, lambda: hd.Csr.from_arrays(*csr))
    fp, fu = forms[True][1], forms[False][1]
    print(fp, fu, int(per_chunk.sum()))
    assert fp["kernel"] == "window" and fp["value_coded"] and fp["vc_packed"] == slots and fp["blocks"] == per_chunk.size, fp
    assert fu["kernel"] == "window" and fu["value_coded"] and fu["vc_packed"] == 0, fu
    # the 255-entry dictionary of the unpacked form holds the 240 frequent values and 15 rare ones
    assert per_chunk.sum() - 15 * 400 < fu["escapes"] < per_chunk.sum() and fp["escapes"] == fu["escapes"]
    check_products(hd, forms, seed=22, modes=modes)


def test_one_chunk_over_capacity_keeps_the_unpacked_form(hd):
    csr, per_chunk, _ = gen_edges(23, K_ESC_CAP + 1)
    assert per_chunk.max() == K_ESC_CAP + 1 and np.count_nonzero(per_chunk > K_ESC_CAP) == 1
    forms = both_forms(hd, lambda: hd.Csr.from_arrays(*csr))
    for arm in (True, False):
        f = forms[arm][1]
        assert f["kernel"] == "window" and f["value_coded"] and f["vc_packed"] == 0, (arm, f)
    check_products(hd, forms, seed=24)


def gen_wide_chunk(seed, wide):
    """230 000 rows of 5 entries (chunks of 1020 or 1025 entries); columns shared by 256 rows at a time, so a chunk names about ten
    distinct ones -- but for chunk 0 when `wide`: its 1025 entries then name 1025 different columns."""
    rng = np.random.default_rng(seed)
    n = 230000
    rowptr = 5 * np.arange(n + 1, dtype=np.int64)
    r = np.arange(n)
    col = ((r // 256) * 8)[:, None] + np.arange(5)[None, :]
    if wide:
        col[:205] = 5 * r[:205, None] + np.arange(5)[None, :]
    bounds = chunk_bounds(rowptr)
    assert bounds[1] - bounds[0] == 1025
    val, is_rare = _fill_values(rng, rowptr[-1], bounds, {})
    sizes = np.diff(bounds)
    tail_escape = [c for c in np.nonzero(sizes == 1025)[0] if is_rare[bounds[c] + 1024]]
    assert tail_escape, "no chunk whose 1025th entry is an escape"
    return (n, n, rowptr, col.ravel(), val)


def test_chunk_of_more_than_1024_distinct_columns_keeps_the_unpacked_form(hd):
    forms = both_forms(hd, lambda: hd.Csr.from_arrays(*gen_wide_chunk(25, True)))
    for arm in (True, False):
        f = forms[arm][1]
        assert f["kernel"] == "window" and f["value_coded"] and f["vc_packed"] == 0, (arm, f)
    check_products(hd, forms, seed=26)
    # its twin without the wide chunk is packed: the distinct columns of that one chunk were the reason (chunks of 1025 entries, an
    # escape in the 1025th: the kernel's loop past the prefetched entries)
    twin = both_forms(hd, lambda: hd.Csr.from_arrays(*gen_wide_chunk(25, False)))
    assert twin[True][1]["vc_packed"] == 512 and twin[False][1]["vc_packed"] == 0, twin[True][1]
    check_products(hd, twin, seed=26, modes=("plain", "scaled_copy", "resid"))


def test_split_product_takes_the_packed_form_back(hd):
    csr, _, _ = gen_edges(27, K_ESC_CAP)
    forms = both_forms(hd, lambda: hd.Csr.from_arrays(*csr))
    Mp, Mu = forms[True][0], forms[False][0]
    assert forms[True][1]["vc_packed"] == 640
    m = Mp.ncols
    rng = np.random.default_rng(28)
    x = rng.standard_normal(m)
    whole = hd._lib.spmv_mode(Mp, "plain", x)["y"]
    nown = m // 2
    with pack_switch(True):
        fs = hd._lib.csr_form(Mp, nown)
        assert fs["kernel"] == "window" and fs["value_coded"] and fs["vc_packed"] == 0, fs
        a = hd._lib.spmv_mode(Mp, "plain", x, nown=nown)["y"]
        b = hd._lib.spmv_mode(Mu, "plain", x, nown=nown)["y"]
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        # codes, positions and the escape count are those of the operator that never was packed; whole products stay unpacked
        f = hd._lib.csr_form(Mp)
        assert f["vc_packed"] == 0 and f["escapes"] == forms[False][1]["escapes"], f
        again = hd._lib.spmv_mode(Mp, "plain", x)["y"]
    assert np.array_equal(again.view(np.int64), whole.view(np.int64))
    assert np.array_equal(whole.view(np.int64), hd._lib.spmv_mode(Mu, "plain", x)["y"].view(np.int64))
    assert hd._lib.format_bytes(Mp)["spmv"] == hd._lib.format_bytes(Mu)["spmv"]


RANKS = """
import sys, json, numpy as np
sys.path.insert(0, %r)
import os
import hypredrive_amd as hd
from hypredrive_amd import _lib
n = int(sys.argv[1])
yaml = "solver: pcg\\npreconditioner:\\n  preset: poisson\\n"
out = {}
for arm in ("1", "0"):
    os.environ["HDA_VC_PACK"] = arm
    r = _lib.thread_ranks_lap7(2, (n, n, n), (1, 1, 2), yaml, want_x=True)
    x = r.pop("x")
    out[arm] = dict(r, xnorm=float(np.linalg.norm(x)))
    np.save(sys.argv[2] + "/x" + arm + ".npy", x)
    print("== two ranks done, HDA_VC_PACK=" + arm, file=sys.stderr, flush=True)
print(json.dumps(out))
""" % ROOT


def test_two_thread_ranks_keep_the_unpacked_form(hd, tmp_path):
    """Overlapped (split) products on the row-partitioned value-coded P0 / R0: never packed, same numbers whatever the switch says, and
    the one-rank result as in tests/test_gpu_hypredrv.py (iterations within one, solution norms to the stopping tolerance)."""
    env = dict(os.environ, HDA_VERBOSE="1", HDA_THREAD_TRANSPORT="device", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", RANKS, "92", str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert "== two ranks done, HDA_VC_PACK=0" in r.stderr
    assert "value-coded SpMV for" in r.stderr and "packed escapes, D =" not in r.stderr, r.stderr[-3000:]
    from hypredrive_amd import hypredrv
    h = hypredrv.Hypredrv("solver: pcg\npreconditioner:\n  preset: poisson\n")
    h.set_laplacian7((92, 92, 92))
    ref = h.solve()
    one = dict(iters=ref["iters"], norm=h.solution_norm("L2"), l1=h.solution_norm("L1"), linf=h.solution_norm("Linf"))
    a, b = out["1"], out["0"]
    assert a["world"] == 2 and a["converged"] and a["iters_spread"] == 0 and a["overlapped"] > 0
    assert a["iters"] == b["iters"] and a["final_rel"] == b["final_rel"]
    assert np.array_equal(np.load(tmp_path / "x1.npy"), np.load(tmp_path / "x0.npy"))
    assert abs(a["iters"] - one["iters"]) <= 1
    for k in ("norm", "l1", "linf"):
        assert a[k] == pytest.approx(one[k], rel=1e-6), k


# ------------------------------------------------------------------ byte accounting
def test_format_bytes_of_a_packed_operator(hd):
    """codes + positions + distinct-column lists + chunk table of four words + the escaped values, side by side as the kernel reads
    them (no term of 12 bytes per escape); + row pointers, x and y as for every product."""
    csr, per_chunk, bounds = gen_edges(29, K_ESC_CAP)
    n, m, rowptr, col, val = csr
    forms = both_forms(hd, lambda: hd.Csr.from_arrays(*csr))
    assert forms[True][1]["vc_packed"] == 640
    nnz, nw = int(rowptr[-1]), per_chunk.size
    lists = sum(np.unique(col[bounds[c]:bounds[c + 1]]).size for c in range(nw))
    index = 2.0 * nnz + 4.0 * lists
    vectors = 4.0 * (n + 1) + 8.0 * m + 8.0 * n
    assert hd._lib.format_bytes(forms[True][0])["spmv"] == index + 16.0 * nw + 1.0 * nnz + 8.0 * int(per_chunk.sum()) + vectors
    assert hd._lib.format_bytes(forms[False][0])["spmv"] == index + 12.0 * nw + 1.0 * nnz + 8.0 * forms[False][1]["escapes"] + vectors
