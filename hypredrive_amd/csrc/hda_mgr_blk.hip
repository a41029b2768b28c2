// hda_mgr_blk.hip -- MGR block-Jacobi prolongation (prolongation_type blk-jacobi), non-Galerkin coarse grids
// (coarse_level_type non-galerkin, nonglk_max_elmts) and the coarse-grid drop (coarse_th); DESIGN section 12, restated in numpy
// by tests/mgr_blk_reference.py.
//
// F blocks: the owned F points of a level in local order, cut into consecutive groups of b (the last one may be shorter); B = the
// block diagonal of A_FF on them (owned columns only: blocks never cross ranks).  Each block is inverted by LU with partial
// pivoting (pivot = first index of the largest magnitude, rows swapped whole), then the unit vectors are solved for in ascending
// order; a pivot with |u_pp| <= 1e-14 max|B_k| or a non-finite inverse fails the setup.  Two tiers by b, one wavefront per
// block with the block and its inverse in LDS: b <= 8 (576 B per 8 x 9 matrix, 1 200 B per workgroup) and b <= 32
// (17 040 B per workgroup).  Both run the same elementwise operations in
// the same order, so they give the same bits.
//
// W = -B^-1 A_FC: the row pattern of every row of block k is the sorted union of the A_FC patterns of block k's rows (symbolic:
// the C columns of each block gathered, segment-sorted, deduplicated); numeric: per F row, acc_c = sum over the block's rows t
// ascending of inv(i, t) a_tc, w_ic = -acc_c.
//
// Non-Galerkin: A_c = A_CC + Ahat_CF W_B is formed as M P_B with M = the C rows of A, their C entries whole and their F entries cut
// to the nonglk_max_elmts largest magnitudes (ties to the smaller global column; 0 = no cut), and P_B = [W_B; I].
//
// coarse_th: an off-diagonal entry of a reduced operator is dropped when |a_ij| < th max_k |a_ik| (the whole row); the unused
// ghost columns are compacted away afterwards.
#include "hda_amg.h"
#include "hda_comm.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

constexpr double kBlkPivTol = 1e-14;

__global__ __launch_bounds__(256) void k_blk_fmark(int n, const int *__restrict__ cf, int *__restrict__ m)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) m[i] = cf[i] < 0;
}
__global__ __launch_bounds__(256) void k_blk_frow(int n, const int *__restrict__ cf, const int *__restrict__ fidx, int *__restrict__ frow)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && cf[i] < 0) frow[fidx[i]] = i;
}

// one wavefront per block k: extract B_k (owned F columns of the block's rows), LU with partial pivoting, inverse by columns
template <int BM>
__global__ __launch_bounds__(64) void k_blk_inv(int nf, int b, int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                const int *__restrict__ cf, const int *__restrict__ fidx, const int *__restrict__ frow,
                                                double *__restrict__ inv, int *__restrict__ bad)
{
   __shared__ double a[BM][BM + 1];
   __shared__ double x[BM][BM + 1];
   __shared__ int    perm[BM];
   __shared__ int    fail, prow;
   const int k = blockIdx.x, lane = threadIdx.x;
   const int f0 = k * b, m = min(b, nf - f0);
   for (int e = lane; e < BM * BM; e += 64) a[e / BM][e % BM] = 0.0;
   if (lane == 0) fail = 0;
   if (lane < m) perm[lane] = lane;
   __syncthreads();
   if (lane < m)
   { // row `lane` of the block (columns in A's order; a repeated column adds)
      const int r = frow[f0 + lane];
      for (int q = rp[r]; q < rp[r + 1]; q++)
      {
         const int j = cj[q];
         if (j >= n || cf[j] >= 0) continue;
         const int t = fidx[j] - f0;
         if (t >= 0 && t < m) a[lane][t] += v[q];
      }
   }
   __syncthreads();
   __shared__ double bmax;
   if (lane == 0)
   {
      double s = 0.0;
      for (int i = 0; i < m; i++)
         for (int j = 0; j < m; j++) s = fmax(s, fabs(a[i][j]));
      bmax = s;
   }
   __syncthreads();
   for (int c = 0; c < m; c++)
   {
      if (lane == 0)
      { // pivot: first index of the largest magnitude in column c, rows c..m-1
         int    p  = c;
         double pv = fabs(a[c][c]);
         for (int i = c + 1; i < m; i++)
            if (fabs(a[i][c]) > pv) { pv = fabs(a[i][c]); p = i; }
         if (!(pv > kBlkPivTol * bmax)) fail = 1;
         if (p != c) { const int t = perm[c]; perm[c] = perm[p]; perm[p] = t; }
         prow = p;
      }
      __syncthreads();
      if (fail) break;
      const int p = prow;
      if (p != c && lane < m) { const double t = a[c][lane]; a[c][lane] = a[p][lane]; a[p][lane] = t; }
      __syncthreads();
      if (lane > c && lane < m) a[lane][c] = a[lane][c] / a[c][c]; // multipliers l_ic
      __syncthreads();
      if (lane > c && lane < m)
         for (int i = c + 1; i < m; i++) a[i][lane] -= a[i][c] * a[c][lane];
      __syncthreads();
   }
   if (fail)
   {
      if (lane == 0) atomicMin(bad, k);
      return;
   }
   // column j of the inverse: L y = P e_j, U x = y (lane j, its own LDS column)
   bool ok = true;
   if (lane < m)
   {
      const int j = lane;
      for (int i = 0; i < m; i++)
      {
         double s = perm[i] == j ? 1.0 : 0.0;
         for (int t = 0; t < i; t++) s -= a[i][t] * x[t][j];
         x[i][j] = s;
      }
      for (int i = m - 1; i >= 0; i--)
      {
         double s = x[i][j];
         for (int t = i + 1; t < m; t++) s -= a[i][t] * x[t][j];
         x[i][j] = s / a[i][i];
         ok      = ok && isfinite(x[i][j]);
      }
      double *out = inv + (size_t)k * b * b;
      for (int i = 0; i < m; i++) out[i * b + j] = x[i][j];
   }
   if (!ok) atomicMin(bad, k);
}

// symbolic W: per block, the number of A_FC entries of its rows, then the coarse columns themselves
__global__ __launch_bounds__(256) void k_blk_fc_count(int nblk, int nf, int b, const int *__restrict__ rp, const int *__restrict__ cj,
                                                      const int *__restrict__ cf, const int *__restrict__ frow, int *__restrict__ cnt)
{
   const int k = blockIdx.x * 256 + threadIdx.x;
   if (k >= nblk) return;
   int c = 0;
   for (int f = k * b; f < min(nf, (k + 1) * b); f++)
   {
      const int r = frow[f];
      for (int q = rp[r]; q < rp[r + 1]; q++) c += cf[cj[q]] > 0;
   }
   cnt[k] = c;
}
__global__ __launch_bounds__(256) void k_blk_fc_fill(int nblk, int nf, int b, const int *__restrict__ rp, const int *__restrict__ cj,
                                                     const int *__restrict__ cf, const int *__restrict__ cidx, const int *__restrict__ frow,
                                                     const int *__restrict__ urp, int *__restrict__ ucj, double *__restrict__ uv)
{
   const int k = blockIdx.x * 256 + threadIdx.x;
   if (k >= nblk) return;
   int o = urp[k];
   for (int f = k * b; f < min(nf, (k + 1) * b); f++)
   {
      const int r = frow[f];
      for (int q = rp[r]; q < rp[r + 1]; q++)
         if (cf[cj[q]] > 0) { ucj[o] = cidx[cj[q]]; uv[o++] = 0.0; }
   }
}
// sorted segment -> its distinct columns at the front, their number
__global__ __launch_bounds__(256) void k_blk_dedup(int nblk, const int *__restrict__ urp, int *__restrict__ ucj, int *__restrict__ ucnt)
{
   const int k = blockIdx.x * 256 + threadIdx.x;
   if (k >= nblk) return;
   const int s = urp[k], e = urp[k + 1];
   int       o = s;
   for (int q = s; q < e; q++)
      if (q == s || ucj[q] != ucj[q - 1]) ucj[o++] = ucj[q];
   ucnt[k] = o - s;
}
// P = [W; I]: C row -> (cidx, 1); F row -> the union pattern of its block
__global__ __launch_bounds__(256) void k_blk_P_count(int n, int b, const int *__restrict__ cf, const int *__restrict__ fidx, const int *__restrict__ ucnt,
                                                     int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   cnt[i] = cf[i] > 0 ? 1 : ucnt[fidx[i] / b];
}
__global__ __launch_bounds__(256) void k_blk_P_fill(int n, int nf, int b, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                    const int *__restrict__ cf, const int *__restrict__ cidx, const int *__restrict__ fidx,
                                                    const int *__restrict__ frow, const double *__restrict__ inv, const int *__restrict__ urp,
                                                    const int *__restrict__ ucj, const int *__restrict__ prp, int *__restrict__ pcj,
                                                    double *__restrict__ pv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   const int p0 = prp[i], p1 = prp[i + 1];
   if (cf[i] > 0) { pcj[p0] = cidx[i]; pv[p0] = 1.0; return; }
   const int f = fidx[i], k = f / b, il = f - k * b, m = min(b, nf - k * b);
   for (int q = p0; q < p1; q++) { pcj[q] = ucj[urp[k] + (q - p0)]; pv[q] = 0.0; }
   const double *w = inv + (size_t)k * b * b + (size_t)il * b;
   for (int t = 0; t < m; t++)
   {
      const int    r  = frow[k * b + t];
      const double wt = w[t];
      for (int q = rp[r]; q < rp[r + 1]; q++)
      {
         const int j = cj[q];
         if (cf[j] <= 0) continue;
         const int c = cidx[j];
         int       lo = p0, hi = p1 - 1; // c is in the row's sorted union
         while (lo < hi)
         {
            const int mid = (lo + hi) >> 1;
            if (pcj[mid] < c) lo = mid + 1;
            else hi = mid;
         }
         pv[lo] += wt * v[q];
      }
   }
   for (int q = p0; q < p1; q++) pv[q] = -pv[q];
}

// M: the C rows of A with their C entries and the kmax largest-magnitude F entries (ties: smaller global column; kmax 0: all)
__device__ inline bool ng_keep(int rs, int re, const int *__restrict__ cj, const double *__restrict__ v, const int *__restrict__ cf,
                               const long long *__restrict__ gid, int kmax, int q)
{
   const int j = cj[q];
   if (cf[j] > 0 || kmax <= 0) return true;
   const double a = fabs(v[q]);
   int          rank = 0;
   for (int s = rs; s < re && rank < kmax; s++)
   {
      const int js = cj[s];
      if (s == q || cf[js] > 0) continue;
      const double as = fabs(v[s]);
      rank += (as > a) || (as == a && gid[js] < gid[j]);
   }
   return rank < kmax;
}
__global__ __launch_bounds__(256) void k_ng_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                  const int *__restrict__ cf, const int *__restrict__ cidx, const long long *__restrict__ gid, int kmax,
                                                  int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] <= 0) return;
   int c = 0;
   for (int q = rp[i]; q < rp[i + 1]; q++) c += ng_keep(rp[i], rp[i + 1], cj, v, cf, gid, kmax, q);
   cnt[cidx[i]] = c;
}
__global__ __launch_bounds__(256) void k_ng_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                 const int *__restrict__ cf, const int *__restrict__ cidx, const long long *__restrict__ gid, int kmax,
                                                 const int *__restrict__ mrp, int *__restrict__ mcj, double *__restrict__ mv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] <= 0) return;
   int o = mrp[cidx[i]];
   for (int q = rp[i]; q < rp[i + 1]; q++)
      if (ng_keep(rp[i], rp[i + 1], cj, v, cf, gid, kmax, q)) { mcj[o] = cj[q]; mv[o++] = v[q]; }
}

// coarse_th: keep the diagonal and every entry with |a_ij| >= th max_k |a_ik|
__global__ __launch_bounds__(256) void k_th_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v, double th,
                                                  int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double mx = 0.0;
   for (int q = rp[i]; q < rp[i + 1]; q++) mx = fmax(mx, fabs(v[q]));
   const double cut = th * mx;
   int          c   = 0;
   for (int q = rp[i]; q < rp[i + 1]; q++) c += (cj[q] == i) || !(fabs(v[q]) < cut);
   cnt[i] = c;
}
__global__ __launch_bounds__(256) void k_th_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v, double th,
                                                 const int *__restrict__ orp, int *__restrict__ ocj, double *__restrict__ ov)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double mx = 0.0;
   for (int q = rp[i]; q < rp[i + 1]; q++) mx = fmax(mx, fabs(v[q]));
   const double cut = th * mx;
   int          o   = orp[i];
   for (int q = rp[i]; q < rp[i + 1]; q++)
      if ((cj[q] == i) || !(fabs(v[q]) < cut)) { ocj[o] = cj[q]; ov[o++] = v[q]; }
}
__global__ __launch_bounds__(256) void k_ghost_used(int nnz, int nown, const int *__restrict__ cj, int *__restrict__ used)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < nnz && cj[q] >= nown) used[cj[q] - nown] = 1;
}
__global__ __launch_bounds__(256) void k_ghost_remap(int nnz, int nown, const int *__restrict__ map, int *__restrict__ cj)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < nnz && cj[q] >= nown) cj[q] = nown + map[cj[q] - nown];
}

void csr_from_counts(DCsr &M, int nrows, int ncols, DArray<int> &cnt, const char *what)
{
   M.nrows = nrows;
   M.ncols = ncols;
   M.rowptr.alloc((size_t)nrows + 1);
   require_int32_total(nrows, cnt.data(), what);
   exclusive_scan(nrows, cnt.data(), M.rowptr.data(), nullptr);
   HDA_HIP(hipMemcpyAsync(&M.nnz, M.rowptr.data() + nrows, 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   M.col.alloc((size_t)std::max(M.nnz, 1));
   M.val.alloc((size_t)std::max(M.nnz, 1));
}

} // namespace

void mgr_blk_build(const DCsr &A, const int *cf, int b, int level, long long row0, int tier, MgrBlocks &B)
{
   if (b < 1 || b > kMgrBlkMax)
   {
      const std::string msg = "MGR blk-jacobi / non-galerkin: F block size b = " + std::to_string(b) + " (the number of f_dofs labels of level " +
                              std::to_string(level) + ") is above " + std::to_string(kMgrBlkMax) + ", which is not implemented";
      HDA_REQUIRE(false, msg.c_str());
   }
   const int n = A.nrows;
   B.b         = b;
   DArray<int> fm((size_t)n + 1);
   B.fidx.alloc((size_t)n + 1);
   fm.zero();
   if (n) k_blk_fmark<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, cf, fm.data());
   exclusive_scan(n, fm.data(), B.fidx.data(), nullptr);
   HDA_HIP(hipMemcpyAsync(&B.nf, B.fidx.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   B.nblk = ceil_div(B.nf, b);
   B.frow.alloc((size_t)std::max(B.nf, 1));
   if (n) k_blk_frow<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, cf, B.fidx.data(), B.frow.data());
   mgr_blk_invert(A, cf, level, row0, tier, B);
}

void mgr_blk_invert(const DCsr &A, const int *cf, int level, long long row0, int tier, MgrBlocks &B)
{
   const int b = B.b;
   B.inv.alloc((size_t)std::max(B.nblk, 1) * b * b);
   B.inv.zero();
   DArray<int> bad(1);
   const int   big = 0x7fffffff;
   HDA_HIP(hipMemcpyAsync(bad.data(), &big, 4, hipMemcpyHostToDevice, STREAM));
   if (tier == 0) tier = b <= 8 ? 1 : 2;
   HDA_REQUIRE(tier == 2 || b <= 8, "MGR block inverses: the small tier takes b <= 8");
   if (B.nblk)
   {
      if (tier == 1)
         k_blk_inv<8><<<B.nblk, 64, 0, STREAM>>>(B.nf, b, A.nrows, A.rowptr.data(), A.col.data(), A.val.data(), cf, B.fidx.data(), B.frow.data(),
                                                  B.inv.data(), bad.data());
      else
         k_blk_inv<kMgrBlkMax><<<B.nblk, 64, 0, STREAM>>>(B.nf, b, A.nrows, A.rowptr.data(), A.col.data(), A.val.data(), cf, B.fidx.data(),
                                                           B.frow.data(), B.inv.data(), bad.data());
      HDA_HIP(hipGetLastError());
   }
   int k = big;
   HDA_HIP(hipMemcpyAsync(&k, bad.data(), 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   long long failed = k != big; // every rank learns of a failure, so none is left waiting in the next collective
   Comm::world().allreduce_host(&failed, 1, 0);
   if (failed && k == big)
   {
      const std::string msg = "MGR level " + std::to_string(level) + ": an F block of another rank is singular";
      HDA_REQUIRE(false, msg.c_str());
   }
   if (k != big)
   {
      int r = 0;
      HDA_HIP(hipMemcpyAsync(&r, B.frow.data() + (size_t)k * b, 4, hipMemcpyDeviceToHost, STREAM));
      Context::get().sync();
      const std::string msg = "MGR level " + std::to_string(level) + ": the F block starting at global row " + std::to_string(row0 + r) +
                              " is singular (pivot below 1e-14 of its largest entry, or a non-finite inverse)";
      HDA_REQUIRE(false, msg.c_str());
   }
}

void mgr_blk_prolongation(const DCsr &A, const int *cf, const int *cidx, int ncols, const MgrBlocks &B, DCsr &P)
{
   const int n = A.nrows, b = B.b, nblk = B.nblk;
   DCsr      U; // row k: the coarse columns of block k's A_FC entries, sorted, then deduplicated in place
   {
      DArray<int> cnt((size_t)nblk + 1);
      cnt.zero();
      if (nblk) k_blk_fc_count<<<ceil_div(nblk, 256), 256, 0, STREAM>>>(nblk, B.nf, b, A.rowptr.data(), A.col.data(), cf, B.frow.data(), cnt.data());
      csr_from_counts(U, nblk, ncols, cnt, "MGR blk-jacobi union patterns");
      if (nblk)
         k_blk_fc_fill<<<ceil_div(nblk, 256), 256, 0, STREAM>>>(nblk, B.nf, b, A.rowptr.data(), A.col.data(), cf, cidx, B.frow.data(),
                                                                 U.rowptr.data(), U.col.data(), U.val.data());
      sort_rows_segmented(U);
   }
   DArray<int> ucnt((size_t)nblk + 1), cnt((size_t)n + 1);
   if (nblk) k_blk_dedup<<<ceil_div(nblk, 256), 256, 0, STREAM>>>(nblk, U.rowptr.data(), U.col.data(), ucnt.data());
   cnt.zero();
   if (n) k_blk_P_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, b, cf, B.fidx.data(), ucnt.data(), cnt.data());
   csr_from_counts(P, n, ncols, cnt, "MGR transfer operator");
   if (n)
      k_blk_P_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, B.nf, b, A.rowptr.data(), A.col.data(), A.val.data(), cf, cidx, B.fidx.data(), B.frow.data(),
                                                         B.inv.data(), U.rowptr.data(), U.col.data(), P.rowptr.data(), P.col.data(), P.val.data());
   Context::get().sync();
}

void mgr_nongalerkin_rows(const DCsr &A, const int *cf, const int *cidx, int nc, const std::vector<long long> &gids, int kmax, DCsr &M)
{
   const int         n = A.nrows;
   DArray<long long> gid;
   gid.upload(gids.data(), std::max<size_t>(gids.size(), 1));
   DArray<int> cnt((size_t)nc + 1);
   cnt.zero();
   if (n) k_ng_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), cf, cidx, gid.data(), kmax, cnt.data());
   csr_from_counts(M, nc, A.ncols, cnt, "MGR non-Galerkin rows");
   if (n)
      k_ng_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), cf, cidx, gid.data(), kmax, M.rowptr.data(),
                                                      M.col.data(), M.val.data());
   Context::get().sync();
}

void mgr_coarse_drop(DCsr &A, double th, std::vector<long long> *ghosts)
{
   const int n = A.nrows;
   DCsr      O;
   DArray<int> cnt((size_t)n + 1);
   cnt.zero();
   if (n) k_th_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), th, cnt.data());
   csr_from_counts(O, n, A.ncols, cnt, "MGR coarse_th");
   if (n) k_th_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), th, O.rowptr.data(), O.col.data(), O.val.data());
   const int ng = A.ncols - n;
   if (ghosts && ng > 0)
   { // ghost columns no row refers to any more leave the column space; the rest keep their (ascending) order
      DArray<int> used((size_t)ng);
      used.zero();
      if (O.nnz) k_ghost_used<<<ceil_div(O.nnz, 256), 256, 0, STREAM>>>(O.nnz, n, O.col.data(), used.data());
      std::vector<int> hu((size_t)ng), map((size_t)ng, -1);
      HDA_HIP(hipMemcpyAsync(hu.data(), used.data(), 4 * (size_t)ng, hipMemcpyDeviceToHost, STREAM));
      Context::get().sync();
      std::vector<long long> kept;
      for (int g = 0; g < ng; g++)
         if (hu[(size_t)g]) { map[(size_t)g] = (int)kept.size(); kept.push_back((*ghosts)[(size_t)g]); }
      DArray<int> dmap;
      dmap.upload(map.data(), map.size());
      if (O.nnz) k_ghost_remap<<<ceil_div(O.nnz, 256), 256, 0, STREAM>>>(O.nnz, n, dmap.data(), O.col.data());
      O.ncols = n + (int)kept.size();
      *ghosts = kept;
   }
   Context::get().sync();
   A = std::move(O);
}

} // namespace hda
