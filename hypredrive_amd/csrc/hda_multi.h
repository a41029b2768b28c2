// hda_multi.h -- up to 8 right-hand sides through one pass over the operator: SpMM on the plain CSR arrays,
// batched BLAS-1 of the PCG recurrences, the pack / unpack kernels of the interleaved layout.  One rank, one row block, fp64.
//
// Layout.  A multivector of k <= 8 columns is stored INTERLEAVED: element (i, j) at X[i * K + j], K = multi_width(k) the smallest of
// 2, 4, 8 that holds k.  Columns k .. K-1 are padding: zero, inactive, never reported.  A gather of x[col] is then one contiguous
// read of 8 K bytes, and every (col, val) pair is loaded once for all columns.  Callers of the public entries never see this: they
// hand over k separate vectors (vector j at base + j * ld) and multi_pack / multi_unpack convert on the device.
//
// Arithmetic.  Every column is summed in an order that depends on the matrix alone -- lanes per row from the row's length, a fixed
// tree across them, fixed block trees for the dot products -- so a column's bits depend neither on the other columns nor on k.
#pragma once

#include "hda_krylov.h"

namespace hda {

constexpr int kMultiMax = 8;
inline int    multi_width(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : 8; }
// why k right-hand sides are refused, by name; empty = accepted
std::string multi_refusal(int k);

// batched dot slots: kMultiMax x kRedBlocks block partials each (column j at slot + j * kRedBlocks), the tree of dot()
enum MultiSlot : int { MS_SP = 0, MS_GAMMA = 1, MS_RR = 2, MS_TMP = 3, kMultiSlots = 4 };
// K-wide blocks of device scalars (block q, column j at [q * kMultiMax + j]).  <r,z> and <r,r> of an iteration sit side by side and
// alternate by iteration parity, as the Scalar enum of hda_kernels.h keeps them
enum MultiScalar : int { MV_GAMMA0 = 0, MV_RR0 = 1, MV_GAMMA1 = 2, MV_RR1 = 3, MV_SP = 4, MV_BB = 5, MV_ALPHA = 6, MV_BETA = 7, MV_TMP = 8, kMultiScalars = 9 };
struct MultiScratch {
   DArray<double> partials, scalars;
   DArray<int>    active;                  // kMultiMax flags the scalar kernels read
   double        *host_scalars = nullptr;  // pinned mirror of `scalars`
   int           *host_active  = nullptr;  // pinned source of `active`
   double        *slot(int s) { return partials.data() + (size_t)s * kMultiMax * kRedBlocks; }
   double        *block(int q) { return scalars.data() + (size_t)q * kMultiMax; }
   const double  *host(int q) const { return host_scalars + (size_t)q * kMultiMax; }
   static MultiScratch &get();
};

// interleaved (n x K) <- k vectors of n, vector j at src + j * ld (device); columns >= k become zero.  And back: k columns only
void multi_pack(int n, int k, int K, const double *src, long long ld, double *dst);
void multi_unpack(int n, int k, int K, const double *src, double *dst, long long ld);
void multi_copy(int n, int K, const double *X, double *Y);
void multi_zero(int n, int K, double *X);
// columns named by the bits of `mask`: Y(:, j) = X(:, j)
void multi_copy_columns(int n, int K, unsigned mask, const double *X, double *Y);
// Z(i, :) = d[i] * R(i, :): the first Jacobi sweep from a zero guess
void multi_scale(int n, int K, const double *d, const double *R, double *Z);

// ---- SpMM on DCsr::rowptr / col / val.  Modes as the single product's:
//   MM_PLAIN   Out = alpha A X + beta Yin   (Yin may be Out; beta == 0 never reads it)
//   MM_RESID   Out = B - A X
//   MM_JACOBI  Out = X + d .* (B - A X), one divisor per row for all columns (Out must not be X)
// W != null: block partials of <W_j, Out_j> into dot_slot.  X has ncols rows, every other operand nrows.
// Algorithmic bytes: 12 nnz + 4 (n + 1) + 8 K ncols + 8 K n, plus 8 K n per further vector operand (spmm_bytes).
enum { MM_PLAIN = 0, MM_RESID = 1, MM_JACOBI = 2 };
void   spmm(const DCsr &A, int K, int mode, double alpha, const double *X, double beta, const double *Yin, const double *B, const double *d,
            const double *W, double *Out, int dot_slot);
double spmm_bytes(const DCsr &A, int K, int mode, bool dot);

// ---- batched BLAS-1
void multi_dot(int n, int K, const double *X, const double *Y, int slot);        // K inner products: partials only
void multi_finalize(int K, int first_slot, int nslots, int first_block);         // scalar block (first_block + s) = sums of slot (first_slot + s)
// alpha_j = active_j ? gamma_j / <s,p>_j : 0 with <s,p> finished from slot MS_SP into block MV_SP (0 also where <s,p> is 0 or not finite)
void multi_cg_alpha(int K, int gamma_block);
// <r,z> and <r,r> finished from MS_GAMMA, MS_RR into blocks gn, gn + 1; beta_j = (active_j and alpha_j != 0) ? gamma_new_j / gamma_old_j : 0
void multi_cg_beta(int K, int gamma_old_block, int gamma_new_block);
// X += alpha_j P, R -= alpha_j S, partials of <r_j, r_j> into rr_slot; a column with alpha_j == 0 keeps the bits of X and R
void multi_cg_update(int n, int K, const double *alpha, const double *P, const double *S, double *X, double *R, int rr_slot);
// P = Z + beta_j P
void multi_cg_dir(int n, int K, const double *beta, const double *Z, double *P);
// scalar block `block`, column j = active_j ? in[j] : 0 (in: K device doubles): caller-given alpha or beta through the scalar kernel
void multi_masked(int K, const double *in, int block);
void multi_set_active(const int *flags);                  // kMultiMax host flags -> MultiScratch::active
void multi_read_scalars_async(int first_block, int nblocks); // -> host_scalars, records Context::ev

// dense coarse solve on K columns: X = inv * F with the column-major inverse of dense_apply
void multi_dense_apply(int n, int K, const double *invT, const double *F, double *X);

// ---- k PCG recurrences in lockstep on interleaved vectors (n x K, device); the preconditioner is amg->apply_multi or none.
// Column by column hypre_PCGSolve as pcg() runs it, without its fusions; X holds the initial guesses on entry.
std::vector<KrylovResult> pcg_multi(const DCsr &A, Amg *amg, const KrylovParams &kp, int k, const double *B, double *X);

} // namespace hda
