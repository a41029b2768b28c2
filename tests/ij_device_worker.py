"""Worker of tests/test_gpu_ij_device_ranks.py (launched with torch.distributed.run): every rank assembles its row block of an irregular
M-matrix from DEVICE triplets -- unordered, every entry split into two adds -- and solves; then the same calls through host pointers."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COMM, HOST, DEVICE = 0x44000000, 0, 1


def main(out, n, seed):
    from dist_worker import random_mmatrix
    from hypredrive_amd import DeviceBuffer, _lib
    from hypredrive_amd import dist as hdist
    from hypredrive_amd import hypredrv as hd
    rank, world = hdist.init("staged")
    A = random_mmatrix(seed, n)
    lo, hi = rank * n // world, (rank + 1) * n // world
    blk = A[lo:hi].tocoo()
    rng = np.random.default_rng(100 + rank)
    # v = 0.25 v + 0.75 v as two contributions, the whole list shuffled
    rows = np.r_[blk.row, blk.row].astype(np.int64) + lo
    cols = np.r_[blk.col, blk.col].astype(np.int64)
    vals = np.r_[0.25 * blk.data, 0.75 * blk.data]
    q = rng.permutation(rows.size)
    rows, cols, vals = rows[q], cols[q], vals[q]
    ncols = np.ones(rows.size, dtype=np.int32)
    b = np.ones(hi - lo)
    L = hd.lib()
    res = {}
    for where in ("device", "host"):
        hd._ij_device_sigs(L)
        if where == "device":
            hA = hd.ij_matrix_device(DeviceBuffer.from_numpy(ncols), DeviceBuffer.from_numpy(rows), DeviceBuffer.from_numpy(cols),
                                     DeviceBuffer.from_numpy(vals), lo, hi - 1, lo, hi - 1, add=True)
            hb = hd.ij_vector_device(DeviceBuffer.from_numpy(b), lo)
        else:
            hA, hb = C.c_void_p(), C.c_void_p()
            assert L.HYPRE_IJMatrixCreate(COMM, lo, hi - 1, lo, hi - 1, C.byref(hA)) == 0 and L.HYPRE_IJMatrixInitialize_v2(hA, HOST) == 0
            assert L.HYPRE_IJMatrixAddToValues(hA, rows.size, ncols.ctypes.data, rows.ctypes.data, cols.ctypes.data, vals.ctypes.data) == 0
            assert L.HYPRE_IJVectorCreate(COMM, lo, hi - 1, C.byref(hb)) == 0 and L.HYPRE_IJVectorInitialize_v2(hb, HOST) == 0
            assert L.HYPRE_IJVectorSetValues(hb, hi - lo, None, b.ctypes.data) == 0 and L.HYPRE_IJVectorAssemble(hb) == 0
        hd.ij_matrix_assemble(hA)
        V = _lib.borrow_ij(hA)
        ghosts, nnz = V.ghost_gids.tolist(), V.nnz
        del V
        h = hd.Hypredrv("solver:\n  pcg:\n    relative_tol: 1.0e-8\npreconditioner: amg\n")
        h.set_matrix(hA)
        h.set_rhs(hb)
        h.finish_system()
        r = h.solve()
        res[where] = dict(iters=r["iters"], converged=r["converged"], ghosts=ghosts, nnz=nnz, x=h.solution())
        h.close()
        L.HYPRE_IJMatrixDestroy(hA)
        L.HYPRE_IJVectorDestroy(hb)
    d, s = res["device"], res["host"]
    want = A[lo:hi].tocsr()
    cols_used = np.unique(want.indices)
    json.dump(dict(rank=rank, world=world, iters_device=d["iters"], iters_host=s["iters"], converged=bool(d["converged"] and s["converged"]),
                   ghosts_equal=d["ghosts"] == s["ghosts"], ghosts=len(d["ghosts"]),
                   ghosts_are_the_blocks=d["ghosts"] == cols_used[(cols_used < lo) | (cols_used >= hi)].tolist(),
                   nnz_ok=d["nnz"] == s["nnz"] == want.nnz,
                   rel_diff=float(np.linalg.norm(d["x"] - s["x"]) / np.linalg.norm(s["x"]))), open(f"{out}.r{rank}.json", "w"))
    np.save(f"{out}.x{rank}.npy", d["x"])
    hdist.finalize()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
