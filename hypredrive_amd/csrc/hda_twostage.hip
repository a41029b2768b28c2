// hda_twostage.hip -- two-stage Gauss-Seidel smoother (hypre relaxation types 11 "2gs-it1" / 12 "2gs-it2").
//
// The triangular solve with D + L of a Gauss-Seidel sweep is replaced by the first terms of its Neumann series:
//
//    r = f - A u ;  z0 = dinv .* r ;  u += z0 ;  z_k = -(dinv / weight) .* (L z_{k-1}), u += z_k   (k = 1 .. terms)
//
// with dinv = weight / a_ii (build_dinv, the plain diagonal: the weight scales r only) and L the strictly lower part of the row's block
// of A in local numbering (columns from the row's block start up to the row; from column 0 without row blocks).  Rows are column-sorted (DCsr), so L is one
// contiguous run of every row: [lbeg_i, lend_i), and without blocks lbeg_i is the row start itself.  Ghost columns (>= nrows) lie
// after every owned one and never belong to L.
//
// Kernels: the residual r = f - A u is the existing residual product (every operator format, the halo exchange under it); the L
// passes are new.  Each L pass reads only the L entries in plain CSR, gathers z_{k-1} (the first pass forms z0_j = dinv_j r_j on
// the fly, so z0 is never stored), updates u in place and, when another term follows, writes z_k.  From a zero guess r = f: no
// residual product runs and u is written, not read -- type 11 from zero is one pass over L and the vectors.
#include "hda_amg.h"

#include <algorithm>

namespace hda {

#define STREAM (Context::get().stream)

// L bounds of every row: lend_i = first entry with column >= i; lbeg_i = first entry with column >= the start of the row's block
// (part: nblk + 1 row starts on the device, empty blocks allowed; lbeg is not written without it).  Binary searches: any row length.
__global__ __launch_bounds__(256) void k_ts_bounds(int n, const int *__restrict__ rp, const int *__restrict__ cj, const int *__restrict__ part,
                                                   int nblk, int *__restrict__ lbeg, int *__restrict__ lend)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   auto first_ge = [&](int lo, int hi, int c) { // first k in [lo, hi) with cj[k] >= c
      while (lo < hi)
      {
         const int mid = (lo + hi) >> 1;
         if (cj[mid] < c) lo = mid + 1;
         else hi = mid;
      }
      return lo;
   };
   const int s = rp[i], e = rp[i + 1];
   lend[i]     = first_ge(s, e, i);
   if (part)
   { // block of row i: the last q with part[q] <= i (empty blocks repeat a start; the non-empty one holding i is the last of them)
      int lo = 0, hi = nblk; // part[0] = 0 <= i < part[nblk] = n
      while (lo < hi)
      {
         const int mid = (lo + hi + 1) >> 1;
         if (part[mid] <= i) lo = mid;
         else hi = mid - 1;
      }
      lbeg[i] = first_ge(s, lend[i], part[lo]);
   }
}

// One L pass, LPR lanes per row and two rows in flight per lane group (the pass is bound by the latency of its dependent loads -- row
// bounds, entries, gathers -- so every wave keeps 2 * 64 / LPR rows' worth of them outstanding).  FIRST: the gathered term is
// z0 = dinv .* zin (zin = r, or f from a zero guess), and u takes z0_i + z1_i in that order; otherwise zin is z_{k-1} and u takes z_k.
// ZG (FIRST only): u is the zero vector, written and not read.  STORE: z_k is written to zout (another term follows).  rw = 1 / weight:
// z_k = -(dinv_i (L z_{k-1})_i) rw (weight 1: rw = 1, exact).  Rows are dealt in tiles of 2 * 256 / LPR so that the workgroups of one
// XCD (blockIdx % 8) walk one contiguous eighth of the rows: that XCD's L2 then holds one window of the gathered vector(s).
template <int LPR, bool FIRST, bool ZG, bool STORE>
__device__ __forceinline__ void ts_row_end(int i, double s, const double *__restrict__ dinv, const double *__restrict__ zin, double *__restrict__ u,
                                           double *__restrict__ zout, double rw)
{
   const double di = dinv[i];
   const double zk = -(di * s) * rw;
   if (FIRST)
   {
      const double z0 = di * zin[i];
      u[i]            = ZG ? z0 + zk : (u[i] + z0) + zk;
   }
   else u[i] = u[i] + zk;
   if (STORE) zout[i] = zk;
}
template <int LPR, bool FIRST, bool ZG, bool STORE>
__global__ __launch_bounds__(256) void k_ts_lpass(int n, const int *__restrict__ lbeg, const int *__restrict__ lend, const int *__restrict__ col,
                                                  const double *__restrict__ val, const double *__restrict__ dinv,
                                                  const double *__restrict__ zin, double *__restrict__ u, double *__restrict__ zout, double rw)
{
   constexpr int R    = 256 / LPR; // rows per half tile
   const int     lane = threadIdx.x & (LPR - 1);
   const int     xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
   const int     per  = (((n + 7) >> 3) + 2 * R - 1) / (2 * R) * (2 * R); // rows per XCD, whole tiles
   for (int t = slot; t * 2 * R < per; t += nslot)
   {
      const int i0 = xcd * per + t * 2 * R + (int)(threadIdx.x / LPR), i1 = i0 + R; // (both inside this XCD's rows)
      int       k0 = 0, e0 = 0, k1 = 0, e1 = 0;
      if (i0 < n) { k0 = lbeg[i0] + lane; e0 = lend[i0]; }
      if (i1 < n) { k1 = lbeg[i1] + lane; e1 = lend[i1]; }
      double s0 = 0.0, s1 = 0.0;
      for (; k0 < e0 || k1 < e1; k0 += LPR, k1 += LPR)
      {
         if (k0 < e0)
         {
            const int j = col[k0];
            s0 += val[k0] * (FIRST ? dinv[j] * zin[j] : zin[j]);
         }
         if (k1 < e1)
         {
            const int j = col[k1];
            s1 += val[k1] * (FIRST ? dinv[j] * zin[j] : zin[j]);
         }
      }
#pragma unroll
      for (int o = LPR >> 1; o > 0; o >>= 1)
      {
         s0 += __shfl_xor(s0, o);
         s1 += __shfl_xor(s1, o);
      }
      if (lane == 0)
      {
         if (i0 < n) ts_row_end<LPR, FIRST, ZG, STORE>(i0, s0, dinv, zin, u, zout, rw);
         if (i1 < n) ts_row_end<LPR, FIRST, ZG, STORE>(i1, s1, dinv, zin, u, zout, rw);
      }
   }
}

static int ts_lpr(const DCsr &A)
{ // lanes per row from the average length of L (about half the off-diagonal entries): two to four entries per lane
   const double l = A.nrows ? 0.5 * std::max((double)A.nnz / A.nrows - 1.0, 0.0) : 0.0;
   if (l <= 8.0) return 4;
   if (l <= 24.0) return 8;
   if (l <= 48.0) return 16;
   if (l <= 96.0) return 32;
   return 64;
}

void two_stage_build(const DCsr &A, const std::vector<int> &part, TwoStage &ts)
{
   const int n    = A.nrows;
   const int nblk = (int)part.size() - 1;
   HDA_REQUIRE(nblk <= 1 || (part.front() == 0 && part.back() == n && std::is_sorted(part.begin(), part.end())),
               "two-stage Gauss-Seidel: row blocks must be ascending row starts from 0 to the number of rows");
   ts.lend.alloc((size_t)std::max(n, 1));
   DArray<int> dpart;
   if (nblk > 1)
   {
      ts.lbeg.alloc((size_t)std::max(n, 1));
      dpart.upload(part.data(), part.size());
   }
   else ts.lbeg.release();
   if (n)
      k_ts_bounds<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), nblk > 1 ? dpart.data() : nullptr, nblk,
                                                        nblk > 1 ? ts.lbeg.data() : nullptr, ts.lend.data());
   ts.lpr = ts_lpr(A);
   ts.gen = A.gen;
   ts.nnz = A.nnz;
   Context::get().sync(); // (dpart is released on return)
}

template <int LPR>
static void lpass(const DCsr &A, const TwoStage &ts, const double *dinv, double rw, const double *zin, double *u, double *zout, bool first, bool zg)
{
   const int  n    = A.nrows;
   const int *lbeg = ts.lbeg.size() ? ts.lbeg.data() : A.rowptr.data();
   constexpr int T = 2 * 256 / LPR; // rows per tile
   const int  per  = (((n + 7) >> 3) + T - 1) / T * T;
   const int  grid = 8 * std::max(1, std::min(per / T, 1024)); // a multiple of 8: every XCD gets its share
   const bool st   = zout != nullptr;
#define HDA_TS(F, Z, S) k_ts_lpass<LPR, F, Z, S><<<grid, 256, 0, STREAM>>>(n, lbeg, ts.lend.data(), A.col.data(), A.val.data(), dinv, zin, u, zout, rw)
   if (first)
   {
      if (zg) { if (st) HDA_TS(true, true, true); else HDA_TS(true, true, false); }
      else { if (st) HDA_TS(true, false, true); else HDA_TS(true, false, false); }
   }
   else { if (st) HDA_TS(false, false, true); else HDA_TS(false, false, false); }
#undef HDA_TS
}

void two_stage_sweep(const DCsr &A, const TwoStage &ts, const double *dinv, double weight, const double *b, double *u, double *r, double *z,
                     int terms, bool zero_guess, const HaloPlan *halo)
{
   HDA_REQUIRE(weight != 0.0, "two-stage Gauss-Seidel: relaxation weight 0");
   const double rw = 1.0 / weight;
   HDA_REQUIRE(terms == 1 || terms == 2, "two-stage Gauss-Seidel: 1 (type 11) or 2 (type 12) terms of the series");
   HDA_REQUIRE(ts.gen == A.gen && ts.nnz == A.nnz && ts.lend.size() >= (size_t)std::max(A.nrows, 1),
               "two-stage Gauss-Seidel: L bounds built for another matrix");
   HDA_REQUIRE(terms == 1 || z, "two-stage Gauss-Seidel type 12 needs a work vector for z1");
   if (A.nrows == 0) return;
   const double *src = b;
   if (!zero_guess)
   {
      residual(A, u, b, r, halo);
      src = r;
   }
   for (int k = 1; k <= terms; k++)
   {
      const bool    first = (k == 1);
      const double *zin   = first ? src : z;
      double       *zout  = (k < terms) ? z : nullptr; // (terms = 2: pass 1 writes z1, pass 2 reads it)
      switch (ts.lpr)
      {
         case 4: lpass<4>(A, ts, dinv, rw, zin, u, zout, first, first && zero_guess); break;
         case 8: lpass<8>(A, ts, dinv, rw, zin, u, zout, first, first && zero_guess); break;
         case 16: lpass<16>(A, ts, dinv, rw, zin, u, zout, first, first && zero_guess); break;
         case 32: lpass<32>(A, ts, dinv, rw, zin, u, zout, first, first && zero_guess); break;
         default: lpass<64>(A, ts, dinv, rw, zin, u, zout, first, first && zero_guess); break;
      }
   }
}

} // namespace hda
