"""Two ranks on one GPU: every rank assembles its row block from device triplets (tests/ij_device_worker.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_assemble_their_row_blocks_from_device_triplets(tmp_path):
    """random_mmatrix(7, 400) cut into two row blocks; each rank hands its block over as unordered device triplets, every entry split
    into two adds.  Ghost list and iteration count are those of the same calls through the host path in the same worker, the solution
    agrees to 1e-12 relative -- and solves the system."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_worker import random_mmatrix
    out = str(tmp_path / "res")
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HDA_COMM_TIMEOUT_S="120")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "ij_device_worker.py"), out, "400", "7"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    res = [json.load(open(f"{out}.r{k}.json")) for k in range(2)]
    for k, q in enumerate(res):
        assert q["rank"] == k and q["world"] == 2 and q["converged"]
        assert q["ghosts_equal"] and q["ghosts_are_the_blocks"] and q["ghosts"] > 0 and q["nnz_ok"]
        assert q["iters_device"] == q["iters_host"] == res[0]["iters_device"]
        assert q["rel_diff"] <= 1e-12
    x = np.concatenate([np.load(f"{out}.x{k}.npy") for k in range(2)])
    A = random_mmatrix(7, 400)
    assert np.linalg.norm(A @ x - 1.0) / 20.0 < 1e-7   # ||b|| = sqrt(400); PCG stopped at 1e-8 of it
