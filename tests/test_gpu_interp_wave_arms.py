"""Characterisation of the lane-group interpolation kernel (k_interp_wave) and of the thread kernel beside it, one operator per arm
of the dispatch in amg_interp_extpi.

extended+i (Csr.interp_extpi, type 6) against the oracle: row pointers, columns and values equal exactly.  extended
(Csr.interp_extended, type 14, the PLUSI = false instantiations) against tests/interp_reference.py at the figure of
tests/test_gpu_interp_family.py: pattern identical, values to 1e-13 relative (reordered sums).  Strength
(theta = 0.25) and the PMIS splitting come from the device; (pmax, trunc_factor) runs over PARAMS, whose last two pairs are outside
the lane-group kernel's range (pmax 0 and 17), so every row goes to the thread kernel.

  operator        what it reaches
  lap7 8^3        longest row 7: 8 lanes a row
  stencil9 30x29  longest row 9: 16 lanes a row
  stencil27 8^3   longest row 27: a wavefront a row
  galerkin 12^3   level-1 operator of the 12^3 Laplacian (rap with its own P): a wavefront a row, candidate lists beyond the floor of 16
  lap1d 500       F points whose only strong F neighbour has three entries: the neighbour rows staged in LDS (at most 8 entries in all)
  random_mmatrix  both signs, irregular rows
  arrow           a row of 301 entries (> 256) that k_interp_rowmode leaves to the thread kernel while the rest stay on the lane-group
                  kernel; it is an F point, and two lane-group rows have it as a strong F neighbour (a neighbour row of more than four
                  entries a lane: the general accumulation path)

test_lane_widths reads the widths from the HDA_VERBOSE trace of a child process (the variable is read once per process).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import interp_reference as ir  # noqa: E402
from dist_worker import random_mmatrix  # noqa: E402

PARAMS = [(4, 0.0), (4, 0.2), (16, 0.0), (0, 0.0), (17, 0.0)]
ARROW_HUB = 400


def lap1d(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))


def full_stencil(*dims):
    """every neighbour of the 3^d box coupled by -1, the diagonal 3^d - 1 (9-point in 2-D, 27-point in 3-D)"""
    B = None
    for m in reversed(dims):
        T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(m, m))
        B = T if B is None else sp.kron(T, B)
    A = sp.csr_matrix(3.0 ** len(dims) * sp.identity(B.shape[0]) - B)
    A.sort_indices()
    return A


def arrow():
    """20 x 20 five-point grid (rows 0..399) and a hub (row 400) that depends strongly on 300 grid points; grid points 0..299 depend
    on it weakly, 300..304 strongly.  Diagonally dominant M-matrix, not symmetric."""
    n = ARROW_HUB
    off = lambda m: sp.diags([1.0, 1.0], [-1, 1], shape=(m, m))
    M = sp.lil_matrix((n + 1, n + 1))
    M[:n, :n] = sp.kron(sp.identity(20), off(20)) + sp.kron(off(20), sp.identity(20))
    M[n, :300] = 1.0
    M[:300, n] = 0.01
    M[300:305, n] = 1.0
    M = M.tocsr()
    A = sp.csr_matrix(sp.diags(np.asarray(M.sum(axis=1)).ravel() + 0.5) - M)
    A.sort_indices()
    return A


def galerkin(hd):
    Ah = hd.lap7(12, 12, 12, want_rhs=False)
    sm = Ah.strength(0.25)
    A1 = Ah.rap(Ah.interp_extpi(sm, Ah.pmis(sm), 4, 0.0)).to_scipy()
    A1.sort_indices()
    return A1


OPERATORS = {
    "lap7 8^3": lambda hd: hd.lap7(8, 8, 8, want_rhs=False).to_scipy(),
    "stencil9 30x29": lambda hd: full_stencil(30, 29),
    "stencil27 8^3": lambda hd: full_stencil(8, 8, 8),
    "galerkin 12^3": galerkin,
    "lap1d 500": lambda hd: sp.csr_matrix(lap1d(500)),
    "random_mmatrix": lambda hd: random_mmatrix(3, 1500),
    "arrow": lambda hd: arrow(),
}
WIDTHS = {"lap7 8^3": 8, "stencil9 30x29": 16, "stencil27 8^3": 64, "galerkin 12^3": 64}


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


@functools.lru_cache(maxsize=None)
def case(hd, op):
    """(A, device handle, strength mask, splitting) of an operator: built once, never modified"""
    A = sp.csr_matrix(OPERATORS[op](hd))
    assert A.shape[0] <= 2000
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(0.25)
    return A, Ah, sm, Ah.pmis(sm)


def strong_f_neighbours(A, sm, cf, i):
    k = np.arange(A.indptr[i], A.indptr[i + 1])
    j = A.indices[k]
    return j[(sm[k] != 0) & (cf[j] == -1)]


def test_operators_are_what_the_table_says(hd):
    """longest rows 7 / 9 / 27; lap1d has F rows whose strong F neighbours hold at most 8 entries together; the arrow's hub is an F
    point of more than 256 entries and a strong F neighbour of an F row on the grid"""
    for op, longest in (("lap7 8^3", 7), ("stencil9 30x29", 9), ("stencil27 8^3", 27)):
        assert np.diff(case(hd, op)[0].indptr).max() == longest, op
    assert np.diff(case(hd, "galerkin 12^3")[0].indptr).max() > 16
    A, _, sm, cf = case(hd, "lap1d 500")
    staged = 0
    for i in np.flatnonzero(cf == -1):
        nb = strong_f_neighbours(A, sm, cf, i)
        staged += nb.size > 0 and np.diff(A.indptr)[nb].sum() <= 8
    assert staged > 0
    A, _, sm, cf = case(hd, "arrow")
    assert A.indptr[ARROW_HUB + 1] - A.indptr[ARROW_HUB] == 301 and cf[ARROW_HUB] == -1
    assert any(ARROW_HUB in strong_f_neighbours(A, sm, cf, i) for i in np.flatnonzero(cf[:ARROW_HUB] == -1))


@pytest.mark.parametrize("op", list(OPERATORS))
def test_extpi_equals_oracle(hd, op):
    from oracle import oracle_ffi as orc
    A, Ah, sm, cf = case(hd, op)
    Ao = orc.Csr.from_scipy(A)
    for pmax, tf in PARAMS:
        Pd = Ah.interp_extpi(sm, cf, pmax, tf).to_scipy()
        Po = orc.interp_extpi(Ao, sm, cf, pmax, tf).to_scipy()
        what = (op, pmax, tf)
        assert Pd.shape == Po.shape and np.array_equal(Pd.indptr, Po.indptr) and np.array_equal(Pd.indices, Po.indices), what
        assert np.array_equal(Pd.data.view(np.int64), Po.data.view(np.int64)), what


@pytest.mark.parametrize("op", list(OPERATORS))
def test_extended_matches_reference(hd, op):
    A, Ah, sm, cf = case(hd, op)
    for pmax, tf in PARAMS:
        Pd = Ah.interp_extended(sm, cf, pmax, tf).to_scipy()
        Pr = ir.extended(A, sm, cf, pmax, tf)
        what = (op, pmax, tf)
        assert ir.same_pattern(Pd, Pr), what
        diff = ir.max_rel_diff(Pd, Pr)
        print(what, "max relative difference", diff)
        assert diff <= 1e-13, what


def trace_child():
    """child process of test_lane_widths: one extended+i build per line of the table, a marker in front of each"""
    import hypredrive_amd as h
    for op in WIDTHS:  # (the Galerkin operator's construction runs a build of its own: all of them before the first marker)
        case(h, op)
    for op in WIDTHS:
        _, Ah, sm, cf = case(h, op)
        for pmax in (4, 0, 17):
            sys.stderr.write(f"CASE {op} | {pmax}\n")
            sys.stderr.flush()
            Ah.interp_extpi(sm, cf, pmax, 0.0)


def test_lane_widths(hd):
    """lanes/row= of the "interp: build" trace line: 8, 16 and 64 for the three stencils, 64 with a candidate capacity above 16 for
    the Galerkin operator, 1 (the thread kernel) for pmax 0 and 17"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, HDA_VERBOSE="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    seen, key = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"CASE (.*) \| (\d+)$", line)
        if m:
            key = (m.group(1), int(m.group(2)))
        m = re.search(r"interp: build \(.*lanes/row=(\d+) caps (\d+) (\d+)", line)
        if m and key:
            seen[key], key = tuple(int(x) for x in m.groups()), None
    assert len(seen) == 3 * len(WIDTHS), r.stderr
    for op, lanes in WIDTHS.items():
        assert seen[(op, 4)][0] == lanes and seen[(op, 0)][0] == 1 and seen[(op, 17)][0] == 1, (op, seen)
    assert seen[("galerkin 12^3", 4)][2] > 16, seen


if __name__ == "__main__":
    trace_child()
