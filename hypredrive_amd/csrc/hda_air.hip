// hda_air.hip -- approximate ideal restriction (AIR: restriction_type air_1 / air_2) and the masked divisors
// of the F / C relaxation schedule (relaxation.points: air).
//
// For every C point i of a level's C/F splitting, R's row is (i, 1) plus z on the neighbourhood N(i) of F points, where z solves
//
//    A(N, N)^T z = -A(i, N)^T        (the equations (R A)_{i,k} = 0 for k in N(i))
//
// N(i) = the strong F neighbours of i (air_1), plus their strong F neighbours (air_2), strength |a_ij| >= theta max_{k != i} |a_ik|.
// The local systems are solved exactly (LU with partial pivoting in fp64, first index of the largest magnitude); a pivot below
// 1e-14 max|M| or a non-finite solution turns the row into injection and is counted; with filter_th > 0 entries below
// filter_th max|z| are dropped.
//
// Symbolic pass: per row the strongest off-diagonal magnitude and the number of strong F neighbours (k_air_strong); per C row an
// upper bound of |N(i)| (k_air_ub), a scan, the candidate columns as 64-bit keys (C rank << 32 | column, k_air_fill), one radix sort
// of all keys (a C row's keys stay in its own segment: the rows' key ranges are disjoint and ascending), and a pass that drops the
// duplicates of every sorted segment in place (k_air_dedup).  Numeric pass, tiered by m = |N(i)|:
//    m <= 32   one wavefront per system, M in LDS (k_air_small; the pivot search is a wave-wide max reduction)
//    m <= 88   one 256-thread workgroup per system, M in LDS (k_air_mid)
//    m >  88   one 256-thread workgroup per system, M in a global workspace, in batches of bounded size (k_air_large)
// Every tier gathers M = A(N, N)^T and the right-hand side from A's rows (binary search of each column in the sorted N(i)), eliminates
// the augmented matrix [M | g] row by row and substitutes backwards -- elementwise the same operations in the same order in every
// tier, so all three give the same bits.  k_air_emit compacts the surviving entries and the unit entry into CSR.
#include "hda_amg.h"

#include <cstring> // rocprim's texture iterator calls memset on the host
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>

namespace hda {

#define STREAM (Context::get().stream)

void exclusive_scan64(long n, const int *in, long long *out); // hda_kernels.hip

namespace {

constexpr int    kSmallM  = 32;  // small tier: m <= 32
constexpr int    kSmallS  = 34;  // its LDS row stride (columns 0..m, m = the right-hand side)
constexpr int    kMidM    = 88;  // mid tier: m <= 88 (88 x 89 doubles = 62 656 B of LDS)
constexpr int    kMidS    = 89;
constexpr double kPivTol  = 1e-14;

__global__ __launch_bounds__(256) void k_air_cmark(int n, const int *__restrict__ cf, int *__restrict__ m)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) m[i] = cf[i] > 0;
}
__global__ __launch_bounds__(256) void k_air_cpt(int n, const int *__restrict__ cf, const int *__restrict__ cidx, int *__restrict__ cpt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && cf[i] > 0) cpt[cidx[i]] = i;
}

// restriction strength: thr_i = theta max_{k != i} |a_ik|; nsf_i = number of strong F neighbours of row i
__global__ __launch_bounds__(256) void k_air_strong(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                    const int *__restrict__ cf, double theta, double *__restrict__ thr, int *__restrict__ nsf)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double mx = 0.0;
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (cj[k] != i && cj[k] < n) mx = fmax(mx, fabs(v[k]));
   const double t   = theta * mx;
   int          cnt = 0;
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int c = cj[k];
      if (c != i && c < n && cf[c] < 0 && fabs(v[k]) >= t) cnt++;
   }
   thr[i] = t;
   nsf[i] = cnt;
}

__device__ __forceinline__ bool strong_f(int i, int c, double a, int n, const int *cf, double t)
{
   return c != i && c < n && cf[c] < 0 && fabs(a) >= t;
}

// upper bound of |N(i)| per C row (distance 2: with the duplicates the union removes)
__global__ __launch_bounds__(256) void k_air_ub(int nc, const int *__restrict__ cpt, int n, const int *__restrict__ rp, const int *__restrict__ cj,
                                                const double *__restrict__ v, const int *__restrict__ cf, const double *__restrict__ thr,
                                                const int *__restrict__ nsf, int dist, int *__restrict__ ub)
{
   const int ci = blockIdx.x * 256 + threadIdx.x;
   if (ci >= nc) return;
   const int i = cpt[ci];
   int       u = nsf[i];
   if (dist == 2)
      for (int k = rp[i]; k < rp[i + 1]; k++)
         if (strong_f(i, cj[k], v[k], n, cf, thr[i])) u += nsf[cj[k]];
   ub[ci] = u;
}

__global__ __launch_bounds__(256) void k_air_fill(int nc, const int *__restrict__ cpt, int n, const int *__restrict__ rp, const int *__restrict__ cj,
                                                  const double *__restrict__ v, const int *__restrict__ cf, const double *__restrict__ thr, int dist,
                                                  const long long *__restrict__ off, unsigned long long *__restrict__ keys)
{
   const int ci = blockIdx.x * 256 + threadIdx.x;
   if (ci >= nc) return;
   const int                i  = cpt[ci];
   const unsigned long long hi = (unsigned long long)ci << 32;
   long long                w  = off[ci];
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int j = cj[k];
      if (!strong_f(i, j, v[k], n, cf, thr[i])) continue;
      keys[w++] = hi | (unsigned)j;
      if (dist == 2)
         for (int q = rp[j]; q < rp[j + 1]; q++)
            if (strong_f(j, cj[q], v[q], n, cf, thr[j])) keys[w++] = hi | (unsigned)cj[q];
   }
}

// sorted segment -> its distinct columns at the segment's start; m = their number
__global__ __launch_bounds__(256) void k_air_dedup(int nc, const long long *__restrict__ off, const unsigned long long *__restrict__ keys,
                                                   int *__restrict__ ncol, int *__restrict__ mm)
{
   const int ci = blockIdx.x * 256 + threadIdx.x;
   if (ci >= nc) return;
   const long long s = off[ci], e = off[ci + 1];
   int             m = 0, last = -1;
   for (long long q = s; q < e; q++)
   {
      const int c = (int)(keys[q] & 0xffffffffu);
      if (c != last) ncol[s + m++] = c;
      last = c;
   }
   mm[ci] = m;
}

__device__ __forceinline__ int find_col(const int *N, int m, int c)
{
   int lo = 0, hi = m;
   while (lo < hi)
   {
      const int mid = (lo + hi) >> 1;
      if (N[mid] < c) lo = mid + 1;
      else hi = mid;
   }
   return (lo < m && N[lo] == c) ? lo : -1;
}

// (value, index) of the largest magnitude, the first index on ties: a wave-wide reduction
__device__ __forceinline__ void wave_argmax(double &val, int &idx)
{
   for (int o = 32; o > 0; o >>= 1)
   {
      const double ov = __shfl_xor(val, o);
      const int    oi = __shfl_xor(idx, o);
      if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
   }
}
__device__ __forceinline__ double wave_max(double v)
{
   for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
   return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
   for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}

struct SysArgs {
   const int       *list, *cpt, *mm, *ncol, *rp, *cj;
   const long long *off;
   const double    *v;
   double          *z;
   unsigned char   *keep;
   int             *fb, *nkeep;
   double           phi;
   int              cnt;
};

// small tier: one wavefront (a 64-thread workgroup) per system, lane p owns row p of [M | g]
__global__ __launch_bounds__(64) void k_air_small(SysArgs a)
{
   __shared__ double sM[kSmallM * kSmallS];
   const int t = blockIdx.x;
   if (t >= a.cnt) return;
   const int  lane = threadIdx.x;
   const int  ci = a.list[t], i = a.cpt[ci], m = a.mm[ci];
   const int *N  = a.ncol + a.off[ci];
   double    *z  = a.z + a.off[ci];
   auto       M  = [&](int p, int q) -> double & { return sM[p * kSmallS + q]; };
   for (int e = lane; e < m * kSmallS; e += 64) sM[e] = 0.0;
   __syncthreads();
   if (lane < m)
   { // column q = lane: row N_q of A (M_pq = a_{N_q N_p})
      const int r = N[lane];
      for (int k = a.rp[r]; k < a.rp[r + 1]; k++)
      {
         const int p = find_col(N, m, a.cj[k]);
         if (p >= 0) M(p, lane) = a.v[k];
      }
   }
   for (int k = a.rp[i] + lane; k < a.rp[i + 1]; k += 64)
   {
      const int p = find_col(N, m, a.cj[k]);
      if (p >= 0) M(p, m) = -a.v[k];
   }
   __syncthreads();
   double mx = 0.0;
   if (lane < m)
      for (int q = 0; q < m; q++) mx = fmax(mx, fabs(M(lane, q)));
   mx               = wave_max(mx);
   const double tol = kPivTol * mx;
   bool         ok  = true;
   for (int k = 0; k < m && ok; k++)
   {
      double pv = (lane >= k && lane < m) ? fabs(M(lane, k)) : -1.0;
      int    pi = lane;
      wave_argmax(pv, pi);
      if (!(pv > tol)) { ok = false; break; }
      if (pi != k && lane >= k && lane <= m)
      {
         const double x = M(k, lane);
         M(k, lane)      = M(pi, lane);
         M(pi, lane)     = x;
      }
      __syncthreads();
      if (lane > k && lane < m)
      {
         const double l = M(lane, k) / M(k, k);
         for (int j = k + 1; j <= m; j++) M(lane, j) = M(lane, j) - l * M(k, j);
      }
      __syncthreads();
   }
   bool finite = true;
   if (ok)
   {
      for (int k = m - 1; k >= 0; k--)
      {
         const double xk = M(k, m) / M(k, k);
         __syncthreads();
         if (lane < k) M(lane, m) = M(lane, m) - M(lane, k) * xk;
         if (lane == k) M(k, m) = xk;
         __syncthreads();
      }
      const double zi = lane < m ? M(lane, m) : 0.0;
      finite          = wave_sum(lane < m && !isfinite(zi) ? 1 : 0) == 0;
   }
   const bool   good = ok && finite;
   const double zi   = (good && lane < m) ? M(lane, m) : 0.0;
   const double zmax = wave_max(fabs(zi));
   const bool   kp   = good && lane < m && (!(a.phi > 0.0) || fabs(zi) >= a.phi * zmax);
   if (lane < m) { z[lane] = kp ? zi : 0.0; a.keep[a.off[ci] + lane] = kp; }
   const int nk = wave_sum(kp ? 1 : 0);
   if (lane == 0) { a.fb[ci] = good ? 0 : 1; a.nkeep[ci] = nk + 1; }
}

// mid / large tier body: one 256-thread workgroup, [M | g] at M with row stride S (LDS or global workspace)
__device__ __forceinline__ void block_solve(const SysArgs &a, int ci, double *M, int S, double *red, int *ired)
{
   const int  tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
   const int  i = a.cpt[ci], m = a.mm[ci];
   const int *N = a.ncol + a.off[ci];
   double    *z = a.z + a.off[ci];
   for (long e = tid; e < (long)m * S; e += 256) M[e] = 0.0;
   __syncthreads();
   for (int q = tid; q < m; q += 256)
   {
      const int r = N[q];
      for (int k = a.rp[r]; k < a.rp[r + 1]; k++)
      {
         const int p = find_col(N, m, a.cj[k]);
         if (p >= 0) M[(long)p * S + q] = a.v[k];
      }
   }
   for (int k = a.rp[i] + tid; k < a.rp[i + 1]; k += 256)
   {
      const int p = find_col(N, m, a.cj[k]);
      if (p >= 0) M[(long)p * S + m] = -a.v[k];
   }
   __syncthreads();
   double mx = 0.0;
   for (long e = tid; e < (long)m * m; e += 256) mx = fmax(mx, fabs(M[(e / m) * S + e % m]));
   mx = wave_max(mx);
   if (lane == 0) red[wid] = mx;
   __syncthreads();
   const double tol = kPivTol * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
   __syncthreads();
   bool ok = true;
   for (int k = 0; k < m; k++)
   {
      if (wid == 0)
      {
         double pv = -1.0;
         int    pi = m;
         for (int p = k + lane; p < m; p += 64)
         {
            const double x = fabs(M[(long)p * S + k]);
            if (x > pv) { pv = x; pi = p; }
         }
         wave_argmax(pv, pi);
         if (lane == 0) { ired[0] = (pv > tol) ? pi : -1; }
      }
      __syncthreads();
      const int piv = ired[0];
      if (piv < 0) { ok = false; break; } // (uniform: every thread read the same word)
      if (piv != k)
         for (int j = k + tid; j <= m; j += 256)
         {
            const double x       = M[(long)k * S + j];
            M[(long)k * S + j]   = M[(long)piv * S + j];
            M[(long)piv * S + j] = x;
         }
      __syncthreads();
      const int  rows = m - k - 1, cols = m - k; // rows k+1..m-1, columns k+1..m
      const long tot  = (long)rows * cols;
      for (long e = tid; e < tot; e += 256)
      {
         const int    p = k + 1 + (int)(e / cols), j = k + 1 + (int)(e % cols);
         const double l = M[(long)p * S + k] / M[(long)k * S + k];
         M[(long)p * S + j] = M[(long)p * S + j] - l * M[(long)k * S + j];
      }
      __syncthreads();
   }
   bool finite = true;
   if (ok)
   {
      for (int k = m - 1; k >= 0; k--)
      {
         const double xk = M[(long)k * S + m] / M[(long)k * S + k];
         __syncthreads();
         for (int p = tid; p < k; p += 256) M[(long)p * S + m] = M[(long)p * S + m] - M[(long)p * S + k] * xk;
         if (tid == 0) M[(long)k * S + m] = xk;
         __syncthreads();
      }
      int bad = 0;
      for (int p = tid; p < m; p += 256) bad += !isfinite(M[(long)p * S + m]);
      bad = wave_sum(bad);
      if (lane == 0) ired[1 + wid] = bad;
      __syncthreads();
      finite = (ired[1] + ired[2] + ired[3] + ired[4]) == 0;
      __syncthreads();
   }
   const bool good = ok && finite;
   double     zm   = 0.0;
   if (good)
      for (int p = tid; p < m; p += 256) zm = fmax(zm, fabs(M[(long)p * S + m]));
   zm = wave_max(zm);
   if (lane == 0) red[wid] = zm;
   __syncthreads();
   const double zmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
   int          nk   = 0;
   for (int p = tid; p < m; p += 256)
   {
      const double zi = good ? M[(long)p * S + m] : 0.0;
      const bool   kp = good && (!(a.phi > 0.0) || fabs(zi) >= a.phi * zmax);
      z[p]                   = kp ? zi : 0.0;
      a.keep[a.off[ci] + p]  = kp;
      nk += kp;
   }
   nk = wave_sum(nk);
   if (lane == 0) ired[5 + wid] = nk;
   __syncthreads();
   if (tid == 0)
   {
      a.fb[ci]    = good ? 0 : 1;
      a.nkeep[ci] = ired[5] + ired[6] + ired[7] + ired[8] + 1;
   }
}

__global__ __launch_bounds__(256) void k_air_mid(SysArgs a)
{
   __shared__ double sM[kMidM * kMidS];
   __shared__ double red[4];
   __shared__ int    ired[9];
   if ((int)blockIdx.x >= a.cnt) return;
   block_solve(a, a.list[blockIdx.x], sM, kMidS, red, ired);
}

__global__ __launch_bounds__(256) void k_air_large(SysArgs a, double *__restrict__ ws, const long long *__restrict__ wsoff)
{
   __shared__ double red[4];
   __shared__ int    ired[9];
   if ((int)blockIdx.x >= a.cnt) return;
   const int ci = a.list[blockIdx.x];
   block_solve(a, ci, ws + wsoff[blockIdx.x], a.mm[ci] + 1, red, ired);
}

// R's rows: the kept (N_p, z_p) and (i, 1), columns ascending
__global__ __launch_bounds__(256) void k_air_emit(int nc, const int *__restrict__ cpt, const long long *__restrict__ off, const int *__restrict__ mm,
                                                  const int *__restrict__ ncol, const double *__restrict__ z, const unsigned char *__restrict__ keep,
                                                  const int *__restrict__ rrp, int *__restrict__ rcj, double *__restrict__ rv)
{
   const int ci = blockIdx.x * 256 + threadIdx.x;
   if (ci >= nc) return;
   const int       i = cpt[ci], m = mm[ci];
   const long long s = off[ci];
   int             w = rrp[ci];
   bool            unit = false;
   for (int p = 0; p < m; p++)
   {
      if (!keep[s + p]) continue;
      const int c = ncol[s + p];
      if (!unit && c > i) { rcj[w] = i; rv[w] = 1.0; w++; unit = true; }
      rcj[w] = c;
      rv[w]  = z[s + p];
      w++;
   }
   if (!unit) { rcj[w] = i; rv[w] = 1.0; }
}

// masked divisors: dst_i = src_i where the point belongs to the sweep's set (sel < 0: F points, sel > 0: C points), else 0
__global__ __launch_bounds__(256) void k_air_mask(int n, const int *__restrict__ cf, int sel, const double *__restrict__ src, double *__restrict__ dst)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) dst[i] = ((sel < 0) == (cf[i] < 0)) ? src[i] : 0.0;
}

} // namespace

void air_restriction(const DCsr &A, const int *cf, int distance, double strong_th, double filter_th, DCsr &R, long long stats[5])
{
   HDA_REQUIRE(distance == 1 || distance == 2, "AIR: distance must be 1 (air_1) or 2 (air_2)");
   HDA_REQUIRE(std::isfinite(strong_th) && strong_th >= 0.0, "AIR: restrict_strong_th must be a finite number >= 0");
   HDA_REQUIRE(std::isfinite(filter_th) && filter_th >= 0.0, "AIR: restrict_filter_th must be a finite number >= 0");
   const int n = A.nrows;
   for (int q = 0; q < 5; q++) stats[q] = 0;
   DArray<int> mark((size_t)n + 1), cidx((size_t)n + 1);
   if (n) k_air_cmark<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, cf, mark.data());
   exclusive_scan(n, mark.data(), cidx.data(), nullptr);
   int nc = 0;
   HDA_HIP(hipMemcpyAsync(&nc, cidx.data() + n, sizeof(int), hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   R.reset_plan();
   R.nrows = nc;
   R.ncols = n;
   R.rowptr.alloc((size_t)nc + 1);
   if (nc == 0)
   {
      R.rowptr.zero();
      R.nnz = 0;
      R.col.alloc(1);
      R.val.alloc(1);
      return;
   }
   DArray<int>    cpt((size_t)nc), nsf((size_t)n), ub((size_t)nc + 1), mm((size_t)nc + 1), fb((size_t)nc), nkeep((size_t)nc + 1);
   DArray<double> thr((size_t)n);
   DArray<long long> off((size_t)nc + 1);
   const int *rp = A.rowptr.data(), *cj = A.col.data();
   const double *v = A.val.data();
   k_air_cpt<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, cf, cidx.data(), cpt.data());
   k_air_strong<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, rp, cj, v, cf, strong_th, thr.data(), nsf.data());
   k_air_ub<<<ceil_div(nc, 256), 256, 0, STREAM>>>(nc, cpt.data(), n, rp, cj, v, cf, thr.data(), nsf.data(), distance, ub.data());
   exclusive_scan64(nc, ub.data(), off.data());
   long long T = 0;
   HDA_HIP(hipMemcpyAsync(&T, off.data() + nc, sizeof(long long), hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   const size_t Ts = (size_t)std::max(T, 1LL);
   DArray<int>                ncol(Ts);
   DArray<double>             z(Ts);
   DArray<unsigned char>      keep(Ts);
   {
      DArray<unsigned long long> keys(Ts), sorted(Ts);
      k_air_fill<<<ceil_div(nc, 256), 256, 0, STREAM>>>(nc, cpt.data(), n, rp, cj, v, cf, thr.data(), distance, off.data(), keys.data());
      if (T > 0)
      {
         size_t tmp_bytes = 0;
         HDA_ROCPRIM(rocprim::radix_sort_keys(nullptr, tmp_bytes, keys.data(), sorted.data(), (size_t)T, 0, 64, STREAM));
         DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
         HDA_ROCPRIM(rocprim::radix_sort_keys(tmp.data(), tmp_bytes, keys.data(), sorted.data(), (size_t)T, 0, 64, STREAM));
      }
      k_air_dedup<<<ceil_div(nc, 256), 256, 0, STREAM>>>(nc, off.data(), sorted.data(), ncol.data(), mm.data());
   }
   // tiers by m (host lists: the large tier's workspace is laid out from them)
   const std::vector<int> hm = mm.to_host();
   std::vector<int>       small, mid, large;
   int                    maxm = 0;
   for (int ci = 0; ci < nc; ci++)
   {
      const int m = hm[(size_t)ci];
      maxm        = std::max(maxm, m);
      (m <= kSmallM ? small : m <= kMidM ? mid : large).push_back(ci);
   }
   SysArgs a;
   a.cpt = cpt.data(); a.mm = mm.data(); a.ncol = ncol.data(); a.rp = rp; a.cj = cj; a.off = off.data(); a.v = v;
   a.z = z.data(); a.keep = keep.data(); a.fb = fb.data(); a.nkeep = nkeep.data(); a.phi = filter_th;
   DArray<int> lsmall, lmid, llarge;
   if (!small.empty())
   {
      lsmall.upload(small.data(), small.size());
      a.list = lsmall.data(); a.cnt = (int)small.size();
      k_air_small<<<a.cnt, 64, 0, STREAM>>>(a);
   }
   if (!mid.empty())
   {
      lmid.upload(mid.data(), mid.size());
      a.list = lmid.data(); a.cnt = (int)mid.size();
      k_air_mid<<<a.cnt, 256, 0, STREAM>>>(a);
   }
   if (!large.empty())
   { // batches whose workspaces together stay below a budget (one system alone may exceed it)
      static const long long budget = getenv("HDA_AIR_WS_DOUBLES") ? atoll(getenv("HDA_AIR_WS_DOUBLES")) : (32LL << 20);
      llarge.upload(large.data(), large.size());
      size_t b0 = 0;
      while (b0 < large.size())
      {
         std::vector<long long> wo;
         long long              tot = 0;
         size_t                 b1  = b0;
         while (b1 < large.size())
         {
            const long long m  = hm[(size_t)large[b1]];
            const long long sz = m * (m + 1);
            if (b1 > b0 && tot + sz > budget) break;
            wo.push_back(tot);
            tot += sz;
            b1++;
         }
         DArray<long long> dwo;
         dwo.upload(wo.data(), wo.size());
         DArray<double> ws((size_t)tot);
         a.list = llarge.data() + b0; a.cnt = (int)(b1 - b0);
         k_air_large<<<a.cnt, 256, 0, STREAM>>>(a, ws.data(), dwo.data());
         Context::get().sync(); // (the workspace is released at the end of the batch)
         b0 = b1;
      }
   }
   exclusive_scan(nc, nkeep.data(), R.rowptr.data(), nullptr);
   int nnz = 0;
   HDA_HIP(hipMemcpyAsync(&nnz, R.rowptr.data() + nc, sizeof(int), hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   R.nnz = nnz;
   R.col.alloc((size_t)std::max(nnz, 1));
   R.val.alloc((size_t)std::max(nnz, 1));
   k_air_emit<<<ceil_div(nc, 256), 256, 0, STREAM>>>(nc, cpt.data(), off.data(), mm.data(), ncol.data(), z.data(), keep.data(), R.rowptr.data(),
                                                      R.col.data(), R.val.data());
   const std::vector<int> hfb = fb.to_host();
   long long              nfb = 0;
   for (int q = 0; q < nc; q++) nfb += hfb[(size_t)q];
   stats[0] = nfb;
   stats[1] = maxm;
   stats[2] = (long long)small.size();
   stats[3] = (long long)mid.size();
   stats[4] = (long long)large.size();
}

void air_mask_divisors(int n, const int *cf, int sel, const double *src, DArray<double> &dst)
{
   dst.alloc((size_t)std::max(n, 1));
   if (n) k_air_mask<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, cf, sel, src, dst.data());
}

} // namespace hda
