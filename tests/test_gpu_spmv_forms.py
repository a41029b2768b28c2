"""Every storage form of the sparse product, in every product mode, against the exact row-by-row reference of
tests/spmv_reference.py.

Each case builds an operator whose CONTENT selects the form (no switches), asserts through hda_csr_form that the whole product and
the split products take the intended kernel, and then runs the grid
    {plain (alpha, beta) in (1, 0), (-1, 1), (2.5, -0.5), yin separate and in place; residual; Jacobi; plain + dot; Jacobi + dot;
     scaled copy} x {whole; split with nown = 0, a middle column, ncols}   (no split on the lane-group form: it has none)
checking
  - the stencil-coded and row-class forms, and every split product at nown = 0 (its owned part is exactly zero, so only k_offd_fix
    adds), bit for bit against the sequential emulation;
  - every other result row by row against the componentwise bound, every fused dot against its bound;
  - y2 == dinv2 * y bit for bit where the scaled-copy epilogue is taken -- exactly on whole products of the lane-group, streamed and
    windowed forms -- and y2 untouched elsewhere;
  - beta = 0 with NaN in yin (never read), and a repeated call bit for bit equal to the first.
Values and x span many decades across rows, so one wrong row fails its own bound however small it is next to the others.

Case x form (LG lane-group k_spmv, ST streamed, WL / WR windowed list / run form, VS / VW value-coded streamed / windowed,
CO stencil entry-coded, RC row-class; split products run on the form's SPLIT kernel, LG's on ST):

| case                                                           | LG | ST | WL | WR | VS | VW | CO | RC |
|----------------------------------------------------------------|----|----|----|----|----|----|----|----|
| generic random operator                                        | x  | x  | x  | x  |    |    |    |    |
| lane-group widths: average rows 3, 8, 15, 30, 60 (lpr 4 .. 64) | x  |    |    |    |    |    |    |    |
| empty rows, first rows of chunks / windows and last rows       | x  | x  | x  |    |    |    | x  | x  |
| nrows not a multiple of 8 * 256; P-shaped (tall), R-shaped     | x  | x  |    | x  |    |    |    |    |
| rows of exactly 1024 entries (kMaxRowLds), several in a row    |    | x  | x  |    |    |    |    |    |
| rows of 1025 and 4000 entries above small_nnz (split refused)  | x  |    |    |    |    |    |    |    |
| 16 column runs per chunk / 17                                  |    |    | x  | x  |    |    |    |    |
| 255 distinct values (no escapes)                               |    |    |    |    | x  | x  |    |    |
| 256 distinct values (one escaping value)                       |    |    |    |    | x  | x  |    |    |
| escapes just under 30 %                                        |    |    |    |    | x  | x  |    |    |
| +0.0, -0.0 and subnormal values                                |    |    |    |    | x  | x  |    |    |
| 7-point stencil                                                |    |    |    |    |    |    |    | x  |
| stencil escapes just under 1/16                                |    |    |    |    |    |    | x  |    |
| 27-point stencil with escapes (several 8-entry batches)        |    |    |    |    |    |    | x  |    |
| 255 (offset, value) pairs, slot 254 in a row of <= 8 entries   |    |    |    |    |    |    |    | x  |
| 256 pairs (one escaping pair)                                  |    |    |    |    |    |    |    | x  |
| 127 row classes / 128                                          |    |    |    |    |    |    | x  | x  |
| CSR rows exactly 1/8 of the rows / one more                    |    |    |    |    |    |    | x  | x  |
| split with ghost columns at a constant offset (dictionary)     |    |    |    |    |    |    | x  | x  |

With rows of at most kMaxRowLds entries every window of 1024 entries holds a row start; rows of exactly 1024 entries put window
starts in the middle of rows and fill the product buffer (kWChunk + maxrow) to the last slot.
"""
import numpy as np
import pytest

import spmv_reference as R

pytestmark = pytest.mark.gpu

LG, ST, WL, WR, CO, RC = "lane_group", "stream", "window", "window_runs", "coded", "rowclass"


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as hd
    if hd.device_count() < 1:
        pytest.skip("needs a HIP device")
    return hd


# ------------------------------------------------------------------ generators (vectorised)
def _rng(seed):
    return np.random.default_rng(seed)


def _wide(rng, n, lo=-1.0, hi=1.0):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


def coo_csr(n, m, r, c, v):
    """CSR of the entries (r, c, v); repeated (r, c) keep the first value; rows column-sorted."""
    r, c, v = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(v, np.float64)
    key, idx = np.unique(r * m + c, return_index=True)
    r, c, v = r[idx], c[idx], v[idx]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return rowptr, c, v


def _random_rows(rng, n, m, lens, band=None):
    """Rows of the given lengths, columns uniform over [0, m) or within +-band of the row's diagonal position."""
    r = np.repeat(np.arange(n), lens)
    if band is None:
        c = rng.integers(0, m, r.size)
    else:
        centre = (r * m) // max(n, 1)
        c = np.clip(centre + rng.integers(-band, band + 1, r.size), 0, m - 1)
    return r, c


def _row_scaled(rng, n, r):
    """Values spanning 2 decades inside a row and 16 across rows."""
    return _wide(rng, r.size) * (10.0 ** rng.uniform(-8, 8, n))[r]


def gen_random(seed, n, m, avg, band=None, spread=2):
    rng = _rng(seed)
    lens = rng.integers(max(avg - spread, 0), avg + spread + 1, n)
    r, c = _random_rows(rng, n, m, lens, band)
    return coo_csr(n, m, r, c, _row_scaled(rng, n, r)) + (m,)


def gen_empty_rows(seed, blocks, m, band=None):
    """Blocks of [2 empty rows, 256 rows of 4 entries]: every 1024-entry window and 2048-entry chunk starts with empty rows; 3 empty
    rows close the matrix."""
    rng = _rng(seed)
    lens = np.tile(np.concatenate([[0, 0], np.full(256, 4)]), blocks)
    lens = np.concatenate([lens, [0, 0, 0]])
    n = lens.size
    r = np.repeat(np.arange(n), lens)
    q = np.arange(r.size) % 4  # four distinct columns per row
    if band is None:
        c = np.mod(rng.integers(0, m, n)[r] + q * ((m - 4) // 7), m)
    else:  # one column in each quarter of the band: distinct, with random gaps (many column runs per window)
        c = np.clip((r * m) // n - band + q * (band // 2) + rng.integers(0, band // 2, r.size), 0, m - 1)
    return coo_csr(n, m, r, c, _row_scaled(rng, n, r)) + (m,)


def _stencil(shape, offsets):
    """(r, c, which offset) of a stencil on a grid in lexicographic order."""
    nx, ny, nz = shape
    idx = np.arange(nx * ny * nz)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    rs, cs, ws = [], [], []
    for w, (dx, dy, dz) in enumerate(offsets):
        ok = (i + dx >= 0) & (i + dx < nx) & (j + dy >= 0) & (j + dy < ny) & (k + dz >= 0) & (k + dz < nz)
        rs.append(idx[ok])
        cs.append(idx[ok] + dx + nx * dy + nx * ny * dz)
        ws.append(np.full(int(ok.sum()), w))
    return np.concatenate(rs), np.concatenate(cs), np.concatenate(ws)


P7 = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
P27 = [(a, b, c) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1)]


def gen_stencil(seed, shape, offsets, const=True, escape_frac=0.0):
    """A stencil operator; escape_frac of its entries (all in odd rows) get values of their own.  The dictionary is filled first
    come, first served: with at least 2 * 65536 rows the sampling pass reads the even rows only and claims the stencil's pairs
    before any escape can take a slot (escapes spread over every row would crowd the stencil's own pairs out of the table)."""
    rng = _rng(seed)
    n = int(np.prod(shape))
    r, c, w = _stencil(shape, offsets)
    coef = _wide(rng, len(offsets), -6, 6)
    v = coef[w] if const else _row_scaled(rng, n, r)
    if escape_frac:
        assert n >= 2 * 65536
        hit = (rng.random(r.size) < 2.0 * escape_frac) & (r % 2 == 1)
        v = np.where(hit, _wide(rng, r.size, -6, 6), v)
    return coo_csr(n, n, r, c, v) + (n,)


def gen_value_coded(seed, n, avg, nvals, band=None, rare=0, rare_frac=0.0, special=False):
    """Values drawn from nvals frequent values (+ rare ones): value-coded.  special: the set holds +0.0, -0.0 and subnormals."""
    rng = _rng(seed)
    lens = rng.integers(avg - 1, avg + 2, n)
    r, c = _random_rows(rng, n, n, lens, band)
    freq = _wide(rng, nvals, -8, 8)
    if special:
        freq[:4] = [0.0, -0.0, 5e-324, -2.5e-310]
    v = freq[rng.integers(0, nvals, r.size)]
    if rare:
        pool = _wide(rng, rare, -8, 8)
        hit = rng.random(r.size) < rare_frac
        v = np.where(hit, pool[rng.integers(0, rare, r.size)], v)
    return coo_csr(n, n, r, c, v) + (n,)


def pair_key(v, delta):
    """The library's hash of a stencil dictionary pair (hda_kernels.hip pair_key): restated so a case can place a pair in a given
    slot of the open-addressed table (home slot key % 255; without collisions every pair sits in its home slot)."""
    with np.errstate(over="ignore"):
        h = np.asarray(v, np.float64).view(np.uint64) ^ (np.asarray(delta, np.int64).astype(np.uint32).astype(np.uint64)
                                                           * np.uint64(0x9E3779B97F4A7C15))
        h = h ^ (h >> np.uint64(29))
        h = h * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ (h >> np.uint64(32))
    return np.where(h == np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0), h)


def _tri(n):
    """Entries of the constant operator with offsets 0, 1, 2 (three row classes: interior, the last two rows)."""
    r = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(n - 2)])
    d = np.concatenate([np.zeros(n, np.int64), np.ones(n - 1, np.int64), np.full(n - 2, 2)])
    return r, r + d, d


def gen_rowclass(seed, n, extra_classes=0, csr_rows=0, csr_escapes=False):
    """Offsets 0, 1, 2 with constant values; extra_classes rows re-spell a row with other dictionary values (a class each);
    csr_rows rows of 9 entries (CSR rows of a row-class operator)."""
    rng = _rng(seed)
    main = _wide(rng, 3, -6, 6)
    r, c, d = _tri(n)
    v = main[d]
    alt = _wide(rng, 8, -6, 6)
    if extra_classes:
        rows = np.sort(rng.choice(np.arange(0, n - 2), extra_classes, replace=False))
        combos = rng.permutation(512)[:extra_classes]
        for pos in range(3):
            sel = np.isin(r, rows) & (d == pos)
            which = (combos[np.searchsorted(rows, r[sel])] >> (3 * pos)) & 7
            v[sel] = alt[which] * (1.0 + pos)
    if csr_rows:
        rows = np.sort(rng.choice(np.arange(0, n - 9), csr_rows, replace=False))
        extra_r = np.repeat(rows, 6)
        extra_d = np.tile(np.arange(3, 9), csr_rows)
        ev = main[0] * (extra_d + 1.0)
        if csr_escapes:  # the 8th entry of a row of 9, and a few more, outside the dictionary
            ev = np.where((extra_d == 7) & (extra_r % 3 == 0), _wide(rng, extra_r.size, -6, 6), ev)
        r, c, v = np.concatenate([r, extra_r]), np.concatenate([c, extra_r + extra_d]), np.concatenate([v, ev])
    return coo_csr(n, n, r, c, v) + (n,)


def gen_dict_full(seed, n, npairs):
    """Exactly npairs (offset, value) pairs: 3 main ones (offsets 0, 1, 2) and npairs - 3 extras, each used by one entry of a special
    row (offsets 0, 1, 2) in an odd row, so the sampling pass (even rows) claims the main pairs first.  npairs = 255: the home slots
    of all pairs are distinct, every pair sits in its home slot, and the pair of slot 254 is known.  Returns the CSR, the row that
    holds the slot-254 pair (or None)."""
    rng = _rng(seed)
    r, c, d = _tri(n)
    while True:
        main = _wide(rng, 3, -6, 6)
        ms = pair_key(main, np.arange(3)) % np.uint64(255)
        if len(set(ms.tolist())) == 3 and 254 not in ms.tolist():
            break
    v = main[d]
    nextra = npairs - 3
    per = -(-nextra // 3)
    extras = []  # (delta, value)
    if npairs == 255:
        free = sorted(set(range(255)) - set(ms.tolist()))
        need = {0: 84, 1: 84, 2: 84}
        cand = {dl: _wide(rng, 200000, -6, 6) for dl in range(3)}
        slots = {dl: (pair_key(cand[dl], np.full(cand[dl].size, dl)) % np.uint64(255)).astype(np.int64) for dl in range(3)}
        for s in free:
            for dl in (0, 1, 2):
                if need[dl] == 0:
                    continue
                hit = np.nonzero(slots[dl] == s)[0]
                if hit.size:
                    extras.append((dl, cand[dl][hit[0]], s))
                    need[dl] -= 1
                    break
            else:
                raise AssertionError("no candidate for slot %d" % s)
    else:
        for k in range(nextra):
            extras.append((k % 3, _wide(rng, 1, -6, 6)[0], -1))
    odd = np.arange(1, n - 2, 2)
    srows = np.sort(rng.choice(odd, per, replace=False))
    bydelta = {dl: [e for e in extras if e[0] == dl] for dl in range(3)}
    row254 = None
    for pos in range(3):
        lst = bydelta[pos]
        for q, (dl, val, s) in enumerate(lst):
            row = srows[q]
            sel = (r == row) & (d == pos)
            v[sel] = val
            if s == 254:
                row254 = int(row)
    return coo_csr(n, n, r, c, v) + (n,), row254


def gen_runs(seed, nruns):
    """Rows of 16 entries, 64 rows (one 1024-entry window) per block; per window the distinct columns form nruns runs of 3
    consecutive columns (16: row i takes base + 100 t + i % 3, t < 16; 17: odd rows take t = 1 .. 16)."""
    rng = _rng(seed)
    n = 65536
    r = np.repeat(np.arange(n), 16)
    t = np.tile(np.arange(16), n)
    if nruns == 17:
        t = t + (r % 2)
    base = ((r // 64) * 64) % (n - 1800)
    c = base + 100 * t + (r % 3)
    return coo_csr(n, n, r, c, _row_scaled(rng, n, r)) + (n,)


def gen_long_rows(seed, n, avg, lengths, band=None):
    """A random operator with a run of rows of the given lengths (contiguous columns) in its middle."""
    rng = _rng(seed)
    lens = rng.integers(avg - 2, avg + 3, n)
    r, c = _random_rows(rng, n, n, lens, band)
    at = n // 2
    lr = np.repeat(np.arange(at, at + len(lengths)), lengths)
    lc = np.concatenate([(at + 50 * q + np.arange(L)) % n for q, L in enumerate(lengths)])
    keep = ~np.isin(r, np.arange(at, at + len(lengths)))
    r, c = np.concatenate([r[keep], lr]), np.concatenate([c[keep], lc])
    return coo_csr(n, n, r, c, _row_scaled(rng, n, r)) + (n,)


def gen_rect(seed, n, m, per, shape):
    """P-shaped (tall: columns near i m / n) or R-shaped (wide: scattered around the row's position)."""
    rng = _rng(seed)
    lens = rng.integers(max(per - 1, 1), per + 2, n)
    r = np.repeat(np.arange(n), lens)
    centre = (r * m) // n
    if shape == "P":
        c = np.clip(centre + rng.integers(-1, 2, r.size), 0, m - 1)
    else:
        c = np.clip(centre + rng.integers(-4, 5, r.size) * 3, 0, m - 1)
    return coo_csr(n, m, r, c, _row_scaled(rng, n, r)) + (m,)


# ------------------------------------------------------------------ the check
def _vectors(rng, n, m):
    return dict(x=_wide(rng, m, -4, 4), yin=_wide(rng, n, -4, 4), b=_wide(rng, n, -4, 4),
                dinv=rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 2.0, n), w=_wide(rng, n, -2, 2),
                dinv2=rng.uniform(0.1, 2.0, n), y2=np.full(n, 7.25))


EPILOGUE_FORMS = (LG, ST, WL, WR)
PLAIN_GRID = [(1.0, 0.0), (-1.0, 1.0), (2.5, -0.5)]


def run_case(hd, csr, whole, split=None, mids=None, seed=0, expect=None, split_modes=True):
    """csr = (rowptr, col, val, ncols).  whole / split: the kernel of the whole / split products (split None: no split grid).
    expect: further fields of csr_form(A) to assert."""
    rowptr, col, val, m = csr
    n = len(rowptr) - 1
    A = hd.Csr.from_arrays(n, m, rowptr, col, val)
    f = hd._lib.csr_form(A)
    assert f["kernel"] == whole, f
    for k, v in (expect or {}).items():
        assert (v(f[k]) if callable(v) else f[k] == v), (k, f)
    drp, dcol, dval = A.download()
    rng = _rng(seed + 99)
    V = _vectors(rng, n, m)
    P = R.Problem(drp, dcol, dval, m, V["x"])
    sequential = whole in (CO, RC)
    nowns = [None]
    if split is not None:
        nowns += [0, (mids if mids is not None else m // 2), m]
    for nown in nowns:
        if nown is not None:
            fs = hd._lib.csr_form(A, nown)
            assert fs["kernel"] == split, (nown, fs)
        exact_bits = sequential or nown == 0
        kw_n = dict(nown=-1 if nown is None else nown)
        modes = [("plain", a, bt, ip) for (a, bt) in PLAIN_GRID for ip in (False, True)]
        modes += [(md, 1.0, 0.0, False) for md in ("resid", "jacobi", "plain_dot", "jacobi_dot", "scaled_copy")]
        for mode, alpha, beta, in_place in modes:
            if mode.startswith("jacobi") and n > m:
                continue  # the Jacobi sweep reads x[i] of every row: square-ish operators only
            yin = V["yin"].copy()
            if beta == 0.0:
                yin[:] = np.nan  # beta = 0 never reads yin
            args = dict(x=V["x"], alpha=alpha, beta=beta, yin=yin, in_place=in_place, b=V["b"], dinv=V["dinv"], w=V["w"])
            if mode == "scaled_copy":
                args.update(dinv2=V["dinv2"], y2=V["y2"])
            out = hd._lib.spmv_mode(A, mode, **args, **kw_n)
            y = out["y"]
            tag = (whole, nown, mode, alpha, beta, in_place)
            ekw = dict(alpha=alpha, beta=beta, yin=yin, b=V["b"], dinv=V["dinv"])
            err, tol = R.row_errors(P, y, mode, **ekw)
            bad = np.nonzero(~(err <= tol))[0]
            assert bad.size == 0, (tag, "rows outside the bound", bad[:10], err[bad[:5]], tol[bad[:5]])
            if exact_bits:
                ref = R.emulate(P, mode, nown=nown, **ekw)
                diff = np.nonzero(y.view(np.int64) != ref.view(np.int64))[0]
                assert diff.size == 0, (tag, "not bitwise the sequential emulation", diff[:10], y[diff[:5]], ref[diff[:5]])
            if mode in ("plain_dot", "jacobi_dot"):
                c = V["w"] if mode == "plain_dot" else V["b"]
                derr, dtol = R.dot_error(P, out["dot"], "plain" if mode == "plain_dot" else "jacobi", c, nown=nown, b=V["b"],
                                         dinv=V["dinv"])
                assert derr <= dtol, (tag, "dot", out["dot"], derr, dtol)
            if mode == "scaled_copy":
                want = nown is None and whole in EPILOGUE_FORMS
                assert out["epilogue_taken"] == want, tag
                if want:
                    assert np.array_equal((V["dinv2"] * y).view(np.int64), out["y2"].view(np.int64)), tag
                else:
                    assert np.array_equal(out["y2"], V["y2"]), tag
            if (mode == "plain" and alpha == 2.5 and in_place) or mode == "jacobi_dot":
                again = hd._lib.spmv_mode(A, mode, **args, **kw_n)
                assert np.array_equal(again["y"].view(np.int64), y.view(np.int64)), (tag, "repeat")
                assert again["dot"] == out["dot"] or (np.isnan(again["dot"]) and np.isnan(out["dot"])), (tag, "repeat dot")
    return A, f


# ------------------------------------------------------------------ cases
@pytest.mark.parametrize("avg,lpr", [(3, 4), (8, 8), (15, 16), (30, 32), (60, 64)])
def test_lane_group_widths(hd, avg, lpr):
    n = 16000 - 3 * avg
    run_case(hd, gen_random(avg, n, n, avg), LG, expect=dict(lpr=lpr), seed=avg)


def test_streamed_random(hd):
    n = 300001
    run_case(hd, gen_random(1, n, n, 4), ST, ST, seed=1, expect=dict(value_coded=False))


def test_windowed_list_banded(hd):
    n = 200003
    run_case(hd, gen_random(2, n, n, 6, band=150), WL, WL, seed=2, expect=dict(value_coded=False))


def test_windowed_runs_7pt_random_values(hd):
    run_case(hd, gen_stencil(3, (64, 64, 64), P7, const=False), WR, WR, seed=3)


@pytest.mark.parametrize("form,band,blocks", [(LG, None, 300), (ST, None, 1100), (WL, 100, 1100)])
def test_empty_rows_at_chunk_and_window_starts(hd, form, band, blocks):
    csr = gen_empty_rows(4, blocks, 100000 if form == LG else 300000, band=band)
    run_case(hd, csr, form, None if form == LG else form, seed=4)


@pytest.mark.parametrize("form", [CO, RC])
def test_empty_rows_coded(hd, form):
    """Empty rows (row class 254, or no batch at all in the entry-coded kernel) in a stencil operator."""
    if form == RC:
        (rp, c, v, m) = gen_rowclass(5, 140000)
    else:
        (rp, c, v, m) = gen_stencil(5, (51, 52, 52), P27, escape_frac=0.02)
    lens = np.diff(rp)
    empty = np.arange(0, lens.size, 997)
    keep = ~np.isin(np.repeat(np.arange(lens.size), lens), empty)
    lens[empty] = 0
    rp2 = np.concatenate([[0], np.cumsum(lens)])
    run_case(hd, (rp2, c[keep], v[keep], m), form, form, seed=5)


@pytest.mark.parametrize("shape,n,m,per,form,split", [("P", 123457, 15433, 2, LG, ST), ("P", 600001, 75001, 3, WR, WR),
                                                     ("R", 360007, 2880056, 4, ST, ST), ("R", 40009, 320072, 4, LG, ST)])
def test_rectangular_and_odd_row_counts(hd, shape, n, m, per, form, split):
    run_case(hd, gen_rect(6, n, m, per, shape), form, split, seed=6)


@pytest.mark.parametrize("form,band", [(ST, None), (WL, 150)])
def test_rows_of_exactly_kmaxrowlds(hd, form, band):
    csr = gen_long_rows(7, 200003, 6, [1024] * 8 + [700, 1024, 1024], band=band)
    run_case(hd, csr, form, form, seed=7, expect=dict(maxrow=1024))


def test_rows_longer_than_kmaxrowlds(hd):
    """Rows of 1025 and 4000 entries send a product above small_nnz to the lane-group kernel, which has no split form: a split
    product is refused before anything is launched."""
    csr = gen_long_rows(8, 280001, 4, [1025, 4000, 1025, 1025])
    assert csr[0][-1] > 1000000
    A, f = run_case(hd, csr, LG, seed=8, expect=dict(maxrow=4000))
    assert hd._lib.csr_form(A, 1000)["kernel"] == "none"
    with pytest.raises(hd.LibraryError, match="no split product"):
        hd._lib.spmv_mode(A, "plain", np.ones(A.ncols), nown=1000)


@pytest.mark.parametrize("nruns,form", [(16, WR), (17, WL)])
def test_window_run_limit(hd, nruns, form):
    run_case(hd, gen_runs(9, nruns), form, form, seed=9)


VC_SHAPES = [(ST, None), (WL, 150)]


@pytest.mark.parametrize("form,band", VC_SHAPES)
def test_value_coded_255_values(hd, form, band):
    run_case(hd, gen_value_coded(10, 250007, 5, 255, band), form, form, seed=10, expect=dict(value_coded=True, escapes=0))


@pytest.mark.parametrize("form,band", VC_SHAPES)
def test_value_coded_256_values(hd, form, band):
    """255 frequent values and a rare one: the rare one is the only value left out of the dictionary."""
    csr = gen_value_coded(11, 250007, 5, 255, band, rare=1, rare_frac=0.001)
    uniq, cnt = np.unique(csr[2], return_counts=True)
    assert uniq.size == 256
    rare_count = int(cnt.min())
    run_case(hd, csr, form, form, seed=11, expect=dict(value_coded=True, escapes=rare_count))


@pytest.mark.parametrize("form,band", VC_SHAPES)
def test_value_coded_escapes_just_under_30_percent(hd, form, band):
    csr = gen_value_coded(12, 250007, 5, 255, band, rare=1500, rare_frac=0.285)
    nnz = csr[0][-1]
    run_case(hd, csr, form, form, seed=12, expect=dict(value_coded=True, escapes=lambda e: 0.27 * nnz < e <= 0.30 * nnz))


@pytest.mark.parametrize("form,band", VC_SHAPES)
def test_value_coded_signed_zeros_and_subnormals(hd, form, band):
    run_case(hd, gen_value_coded(13, 250007, 5, 255, band, special=True), form, form, seed=13, expect=dict(value_coded=True, escapes=0))


def test_rowclass_7pt(hd):
    csr = gen_stencil(14, (40, 40, 41), P7)
    run_case(hd, csr, RC, RC, mids=40 * 40 * 20 + 7, seed=14, expect=dict(escapes=0, rc_esc_rows=0))


def test_stencil_escapes_just_under_one_sixteenth(hd):
    csr = gen_stencil(15, (52, 52, 52), P7, escape_frac=0.061)
    nnz = csr[0][-1]
    run_case(hd, csr, CO, CO, seed=15, expect=dict(escapes=lambda e: 0.055 * nnz < e <= nnz / 16))


def test_27pt_with_escapes(hd):
    """27 entries per row: four 8-entry decode batches, escapes at every position of a batch; more than 8 entries per row leaves
    every row a CSR row, so the row-class form is rejected."""
    csr = gen_stencil(16, (51, 52, 52), P27, escape_frac=0.03)
    run_case(hd, csr, CO, CO, mids=51 * 52 * 26 + 5, seed=16, expect=dict(maxrow=27, escapes=lambda e: e > 0))


def test_dictionary_slot_254(hd):
    """255 pairs fill the dictionary; the row that uses slot 254 has 3 entries and must stay a CSR row."""
    csr, row254 = gen_dict_full(17, 140000, 255)
    assert row254 is not None
    run_case(hd, csr, RC, RC, seed=17, expect=dict(escapes=0, rc_esc_rows=1))


def test_dictionary_256_pairs(hd):
    """256 pairs: one extra pair (used by one entry) finds the table full and escapes; its row is a CSR row, and so is the row
    that uses the pair in slot 254 (the same row or another)."""
    csr, _ = gen_dict_full(18, 140000, 256)
    run_case(hd, csr, RC, RC, seed=18, expect=dict(escapes=1, rc_esc_rows=lambda k: k in (1, 2)))


@pytest.mark.parametrize("extra,form", [(124, RC), (125, CO)])
def test_row_class_limit(hd, extra, form):
    """3 classes of the operator + extra re-spelled rows: 127 classes are served by the row-class kernel, 128 are not."""
    run_case(hd, gen_rowclass(19, 140000, extra_classes=extra), form, form, seed=19, expect=dict(escapes=0))


@pytest.mark.parametrize("more,form", [(0, RC), (1, CO)])
def test_csr_rows_one_eighth(hd, more, form):
    """Rows of 9 entries (some with an escape at the 8th entry) are CSR rows: 1/8 of the rows is accepted, one more is not."""
    n = 140000
    csr = gen_rowclass(20, n, csr_rows=n // 8 + more, csr_escapes=True)
    f = dict(rc_esc_rows=n // 8) if form == RC else {}
    run_case(hd, csr, form, form, seed=20, expect=f)
