#!/usr/bin/env python3
"""Write a poromechanics-like stand-in for the reference's poromech2k data set (examples/ex7.yml reads
data/poromech2k/np1/ls_*/{IJ.out.A, IJ.out.b, dofmap.out}; the data set is not in the reference tree): hypre ASCII IJ matrix /
vector parts and dofmap parts, interleaved node-major with 5 labels per node of an n x n x n grid:

    0, 1, 2  displacement: per node a rotated anisotropic tensor T_i = Q_i diag(1, 0.3, 0.1) Q_i^T, edge blocks -(T_i + T_j) / 2,
             so the 3 x 3 nodal blocks are full (on a plain FD / Q1 grid the same-node ux / uy coupling vanishes and blk-jacobi
             would equal jacobi)
    3        a cell-local field coupled only to its own node's displacement and pressure
    4        pressure: 7-point diffusion plus storage, with a Biot-type coupling G (central difference of u, the divergence)
             entering as [K, -G^T; G, L]: a nonsymmetric, positive-real system

np1 and np4 (rows cut at node boundaries) parts go to <dir>/np1 and <dir>/np4.
usage: make_poromech.py <dir> [n=8] [seed=0]"""
import os
import sys

import numpy as np
import scipy.sparse as sp

NLAB = 5


def system(n=8, seed=0):
    """(A, labels): the global stand-in matrix (CSR, rows column-sorted) and its dofmap."""
    rng = np.random.default_rng(seed)
    N = n ** 3
    q, r = np.linalg.qr(rng.standard_normal((N, 3, 3)))
    Q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]        # a random rotation per node
    T = Q @ (np.array([1.0, 0.3, 0.1])[None, :, None] * np.transpose(Q, (0, 2, 1)))
    idx = np.arange(N).reshape(n, n, n)
    rows, cols, vals = [], [], []

    def put(i, j, v):
        i, j, v = np.broadcast_arrays(i, j, np.asarray(v, dtype=np.float64))
        rows.append(i.ravel()), cols.append(j.ravel()), vals.append(v.ravel())

    d3 = np.arange(3)
    for ax in range(3):
        a = np.moveaxis(idx, ax, 0)
        i, j = a[:-1].ravel(), a[1:].ravel()
        K = 0.5 * (T[i] + T[j])                                          # (edges, 3, 3)
        for p, q_, s in ((i, j, -1.0), (j, i, -1.0), (i, i, 1.0), (j, j, 1.0)):
            put(NLAB * p[:, None, None] + d3[None, :, None], NLAB * q_[:, None, None] + d3[None, None, :], s * K)
        # pressure diffusion and Biot coupling along this axis (G: p row, u column; u row gets -G^T)
        for p, q_ in ((i, j), (j, i)):
            put(NLAB * p + 4, NLAB * q_ + 4, -1.0)
            put(NLAB * p + 4, NLAB * p + 4, 1.0)
        g = 0.5
        put(NLAB * i + 4, NLAB * j + ax, g), put(NLAB * j + ax, NLAB * i + 4, -g)
        put(NLAB * j + 4, NLAB * i + ax, -g), put(NLAB * i + ax, NLAB * j + 4, g)
    nodes = np.arange(N)
    c = rng.uniform(0.05, 0.15, (N, 3))
    for d in range(3):
        put(NLAB * nodes + d, NLAB * nodes + d, 0.05)                     # a little mass: K is SPD on the free grid
        put(NLAB * nodes + 3, NLAB * nodes + d, c[:, d]), put(NLAB * nodes + d, NLAB * nodes + 3, c[:, d])
    put(NLAB * nodes + 3, NLAB * nodes + 3, rng.uniform(2.0, 3.0, N))
    put(NLAB * nodes + 3, NLAB * nodes + 4, 0.2), put(NLAB * nodes + 4, NLAB * nodes + 3, 0.1)
    put(NLAB * nodes + 4, NLAB * nodes + 4, 0.1)                         # storage
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(NLAB * N, NLAB * N))
    A.sum_duplicates()
    A.sort_indices()
    return A, np.tile(np.arange(NLAB), N)


def write_parts(A, labels, d, nparts, rhs=None):
    os.makedirs(d, exist_ok=True)
    N = A.shape[0]
    nodes = N // NLAB
    cuts = [NLAB * ((nodes * r) // nparts) for r in range(nparts + 1)]
    rhs = np.ones(N) if rhs is None else rhs
    for r in range(nparts):
        lo, hi = cuts[r], cuts[r + 1]
        with open(os.path.join(d, f"IJ.out.A.{r:05d}"), "w") as f:
            f.write(f"{lo} {hi - 1} {lo} {hi - 1}\n")
            for i in range(lo, hi):
                for k in range(A.indptr[i], A.indptr[i + 1]):
                    f.write(f"{i} {A.indices[k]} {A.data[k]:.17e}\n")
        with open(os.path.join(d, f"IJ.out.b.{r:05d}"), "w") as f:
            f.write(f"{lo} {hi - 1}\n" + "".join(f"{i} {rhs[i]:.17e}\n" for i in range(lo, hi)))
        with open(os.path.join(d, f"dofmap.out.{r:05d}"), "w") as f:
            f.write(f"{hi - lo}\n" + "".join(f"{v}\n" for v in labels[lo:hi]))
    return cuts


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    A, labels = system(n, seed)
    for p in (1, 4):
        write_parts(A, labels, os.path.join(root, f"np{p}"), p)
    print(f"wrote {root}/np1 and np4: {A.shape[0]} rows, {A.nnz} nonzeros, labels 0-4")


if __name__ == "__main__":
    main()
