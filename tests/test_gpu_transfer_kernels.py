"""The level-0 transfer operators (P0, R0) on the value-coded windowed kernel k_spmv_win<0, false, true, ...>.

Two things are pinned here:

  - value coding only changes how the values are stored: plain product, `x += P e` (beta = 1, yin aliasing out) and the product with
    the scaled second result (spmv_with_scaled_copy, its own EPI instantiation of the kernel) agree BIT FOR BIT with the same
    operator applied with HDA_CODED=0, both results;
  - the value-coded form is not dearer than not coding at all: at 256^3 the median of 20 event-timed launches of the P0 and of the
    R0 apply is at most 1.25 x that of the HDA_CODED=0 form.  Recorded ratios: 0.94 - 1.0 while the kernel ran at 0.219 ms (uncoded
    0.232 / 0.222 ms), 1.55 in the records that showed 0.353 ms; 1.25 lies between, far from either by more than the ~1 % same-box
    repeatability, and the two forms run back to back on one GPU so the box cancels.

coded_enabled() reads HDA_CODED once per process, so every arm is a fresh child process that leaves its results in tmp_path; the
children run one after the other, each under a timeout, and a failed child ends the test.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = """
import sys, json, numpy as np
sys.path.insert(0, %r)
import hypredrive_amd as hd
n, out = int(sys.argv[1]), sys.argv[2]
A = hd.lap7(n, n, n)
amg = hd.Amg(A)
ops = dict(P=amg.level_matrix(0, 1), R=amg.level_matrix(0, 2))
""" % ROOT

PRODUCTS = PRELUDE + """
forms = {}
for name, M in ops.items():
    rng = np.random.default_rng(31 + M.ncols)
    x = rng.standard_normal(M.ncols)
    y0 = rng.standard_normal(M.nrows)
    d2 = rng.uniform(0.5, 2.0, M.nrows)
    r = hd._lib.spmv_mode(M, "plain", x)
    np.save(f"{out}/{name}_plain.npy", r["y"])
    r = hd._lib.spmv_mode(M, "plain", x, alpha=1.0, beta=1.0, yin=y0, in_place=True)
    np.save(f"{out}/{name}_add.npy", r["y"])
    r = hd._lib.spmv_mode(M, "scaled_copy", x, dinv2=d2)
    np.save(f"{out}/{name}_scaled_y.npy", r["y"])
    np.save(f"{out}/{name}_scaled_y2.npy", r["y2"])
    f = hd._lib.csr_form(M)
    forms[name] = dict(kernel=f["kernel"], value_coded=f["value_coded"], escapes=f["escapes"], nnz=int(M.nnz), taken=r["epilogue_taken"])
print(json.dumps(forms))
"""

TIMING = PRELUDE + """
res = {}
for name, M in ops.items():
    t = sorted(hd.time_kernel(0, M, None, reps=1)[0] for _ in range(20))
    f = hd._lib.csr_form(M)
    res[name] = dict(median_ms=0.5 * (t[9] + t[10]), min_ms=t[0], max_ms=t[-1], kernel=f["kernel"], value_coded=f["value_coded"])
print(json.dumps(res))
"""

ARMS = (("coded", {}), ("uncoded", {"HDA_CODED": "0"}))
RESULTS = ("plain", "add", "scaled_y", "scaled_y2")


@pytest.fixture(scope="module")
def gpu():
    import hypredrive_amd as hd
    if hd.device_count() < 1:
        pytest.skip("needs a HIP device")
    return hd


def run_child(code, n, out, env, limit):
    os.makedirs(out, exist_ok=True)
    r = subprocess.run([sys.executable, "-c", code, str(n), str(out)], capture_output=True, text=True, env=dict(os.environ, **env),
                       timeout=limit)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("n", [64, 96])
def test_value_coded_transfer_products_equal_uncoded_bit_for_bit(gpu, tmp_path, n):
    forms = {}
    for arm, env in ARMS:
        forms[arm] = run_child(PRODUCTS, n, tmp_path / arm, env, 300)
    print(n, forms)
    for name in ("P", "R"):
        c, u = forms["coded"][name], forms["uncoded"][name]
        assert not u["value_coded"] and c["nnz"] == u["nnz"]
        if c["kernel"] == "window":  # (the second result is written by the windowed kernel itself, in both arms)
            assert c["taken"] and u["taken"]
        for res in RESULTS:
            a = np.load(tmp_path / "coded" / f"{name}_{res}.npy")
            b = np.load(tmp_path / "uncoded" / f"{name}_{res}.npy")
            assert a.shape == b.shape and np.all(np.isfinite(a)) and np.any(a != 0.0)
            assert np.array_equal(a, b), (n, name, res, int(np.sum(a != b)))
    if n == 96:  # (R0 has 1.4 M entries there: the value-coded windowed kernel has really run)
        assert forms["coded"]["R"]["value_coded"] and forms["coded"]["R"]["kernel"] == "window"


def test_value_coded_transfer_kernels_are_not_dearer_than_uncoded(gpu, tmp_path):
    t = {}
    for arm, env in ARMS:
        t[arm] = run_child(TIMING, 256, tmp_path / arm, env, 300)
    for name in ("P", "R"):
        c, u = t["coded"][name], t["uncoded"][name]
        print(f"{name}0 at 256^3: coded {c['median_ms']:.4f} ms ({c['min_ms']:.4f} - {c['max_ms']:.4f}), uncoded {u['median_ms']:.4f} ms "
              f"({u['min_ms']:.4f} - {u['max_ms']:.4f}), ratio {c['median_ms'] / u['median_ms']:.3f}")
    for name in ("P", "R"):
        c, u = t["coded"][name], t["uncoded"][name]
        assert c["kernel"] == "window" and c["value_coded"] and not u["value_coded"]
        assert c["median_ms"] <= 1.25 * u["median_ms"], (name, c, u)
