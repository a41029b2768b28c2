// hda_schwarz.hip -- overlapping Schwarz with ILU(k) subdomain solves: hypre's Schwarz variants "ras-iluk" (10) and "as-iluk" (11) as
// hypredrv_SchwarzCreate configures them (reference src/internal/schwarz.c:20-34, :82-96).  hypre is not part of the reference tree, so
// the arithmetic is restated (tests/schwarz_reference.py is the same definition on the host).  PARITY UNPINNED
// against hypre: no reference output for Schwarz exists.
//
//   blocks      V contiguous row blocks of the n owned rows (the conventions of IluParams::blocks)
//   overlap     Omega_b^0 = rows of block b, Omega_b^(d+1) = Omega_b^d + { j : a_ij stored, i in Omega_b^d }: the stored pattern by
//               rows, explicit zeros count, A is not symmetrised
//   subdomain   A_b = A[Omega_b, Omega_b] in ascending global order; all A_b together are ONE block-diagonal CSR of N_ext rows
//   local solve ILU(k) of A_b: the pattern by a row-parallel search (below), the numbers by hda_ilu.hip on that pattern
//   apply       y = U^-1 L^-1 r[Omega];  ras: z_i = w y_{b(i)}[i];  as: z_i = w sum_b y_b[i] in ascending b -- gathers, no atomics
//
// Symbolic ILU(k), path formulation (Rose-Tarjan fill paths with lengths, Hysom-Pothen): (i, j) has level l exactly when the shortest
// path i -> j in the graph of A_b whose interior vertices are all numbered below min(i, j) has l + 1 edges.  Rows are independent.  A
// row runs a layered search of depth k + 1 from i that expands vertices below i only and keeps, per visited vertex t, the smallest
// "largest interior vertex" m(t) over the paths found so far; t is an entry of the row as soon as some path reaches it with m < t, and
// t is expanded again in the next layer only when its m improved in this one (a longer path with a larger m is dominated).  One
// wavefront per row; visited table, frontier and entry list live in LDS.  A row that visits more than kSchwarzLdsRows vertices is
// redone by the same search on dense arrays in global memory (one set per worker wavefront).  Count pass, scan, fill pass.
#include "hda_amg.h"

#include <cstring> // rocprim's texture iterator calls memset on the host
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

typedef unsigned long long u64;

constexpr int kCap    = kSchwarzLdsRows; // visited vertices of a row in LDS
constexpr int kHash   = 2 * kCap;        // open addressing at load <= 1/2
constexpr int kInf    = 0x7f7f7f7f;      // "no path yet" (what a byte-wise memset writes)
constexpr int kEntry  = 1 << 30, kSeen = 1 << 29;
constexpr int kWorkers = 64; // wavefronts of the global-memory path

// ---------------------------------------------------------------- overlap expansion
// keys: (block << 33) | (row << 1) | candidate bit -- sorted, a member of the current set comes before a candidate of the same (block, row)
__device__ __forceinline__ int sw_block_of(int i, const int *__restrict__ part, int V)
{
   int a = 0, b = V; // part[a] <= i < part[b]
   while (b - a > 1)
   {
      const int m = (a + b) >> 1;
      if (part[m] <= i) a = m;
      else b = m;
   }
   return a;
}
__device__ __forceinline__ int sw_key_row(u64 k) { return (int)((k >> 1) & 0x7fffffffu); }
__device__ __forceinline__ int sw_key_block(u64 k) { return (int)(k >> 33); }

__global__ __launch_bounds__(256) void k_sw_init(int n, const int *__restrict__ part, int V, u64 *__restrict__ keys)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   keys[i] = ((u64)sw_block_of(i, part, V) << 33) | ((u64)i << 1);
}
// entries of the frontier rows that name an owned column
__global__ __launch_bounds__(256) void k_sw_front_count(int nf, const u64 *__restrict__ front, int n, const int *__restrict__ rp,
                                                        const int *__restrict__ cj, int *__restrict__ cnt)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q >= nf) return;
   const int i = sw_key_row(front[q]);
   int       c = 0;
   for (int k = rp[i]; k < rp[i + 1]; k++) c += (cj[k] < n);
   cnt[q] = c;
}
__global__ __launch_bounds__(256) void k_sw_front_fill(int nf, const u64 *__restrict__ front, int n, const int *__restrict__ rp,
                                                       const int *__restrict__ cj, const int *__restrict__ off, u64 *__restrict__ cand)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q >= nf) return;
   const int i = sw_key_row(front[q]);
   const u64 b = (u64)sw_key_block(front[q]) << 33;
   int       o = off[q];
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (cj[k] < n) cand[o++] = b | ((u64)cj[k] << 1) | 1u;
}
// sorted union of set and candidates: head = first of its (block, row); fresh = head that the set did not hold
__global__ __launch_bounds__(256) void k_sw_heads(int m, const u64 *__restrict__ s, int *__restrict__ head, int *__restrict__ fresh)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q >= m) return;
   const int h = (q == 0) || ((s[q] >> 1) != (s[q - 1] >> 1));
   head[q]     = h;
   fresh[q]    = h && (s[q] & 1u);
}
__global__ __launch_bounds__(256) void k_sw_compact(int m, const u64 *__restrict__ s, const int *__restrict__ hpos, const int *__restrict__ fpos,
                                                    u64 *__restrict__ set, u64 *__restrict__ front)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q >= m) return;
   const u64 k = s[q] & ~(u64)1;
   if (hpos[q + 1] > hpos[q]) set[hpos[q]] = k;
   if (fpos[q + 1] > fpos[q]) front[fpos[q]] = k;
}
__global__ __launch_bounds__(256) void k_sw_dom(int next, const u64 *__restrict__ set, int V, int *__restrict__ dom_rows, int *__restrict__ dom_ptr)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < next) dom_rows[q] = sw_key_row(set[q]);
   if (q <= V)
   { // first position whose block is >= q
      int a = 0, b = next;
      while (a < b)
      {
         const int m = (a + b) >> 1;
         if (sw_key_block(set[m]) < q) a = m + 1;
         else b = m;
      }
      dom_ptr[q] = a;
   }
}
// position of column j in the subdomain [lo, hi) of dom_rows, or -1
__device__ __forceinline__ int sw_find(const int *__restrict__ dom_rows, int lo, int hi, int j)
{
   while (lo < hi)
   {
      const int m = (lo + hi) >> 1;
      if (dom_rows[m] < j) lo = m + 1;
      else hi = m;
   }
   return lo;
}
__global__ __launch_bounds__(256) void k_sw_inverse(int n, int next, const int *__restrict__ part, int V, const int *__restrict__ dom_ptr,
                                                    const int *__restrict__ dom_rows, int *__restrict__ own_pos, u64 *__restrict__ keys)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < n)
   {
      const int b = sw_block_of(q, part, V);
      own_pos[q]  = sw_find(dom_rows, dom_ptr[b], dom_ptr[b + 1], q);
   }
   if (q < next) keys[q] = ((u64)dom_rows[q] << 32) | (u64)q; // sorted: the copies of a row in ascending position = ascending subdomain
}
__global__ __launch_bounds__(256) void k_sw_copies(int n, int next, const u64 *__restrict__ skeys, int *__restrict__ copy_ptr, int *__restrict__ copy_pos)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < next) copy_pos[q] = (int)(skeys[q] & 0xffffffffu);
   if (q <= n)
   {
      int a = 0, b = next;
      while (a < b)
      {
         const int m = (a + b) >> 1;
         if ((int)(skeys[m] >> 32) < q) a = m + 1;
         else b = m;
      }
      copy_ptr[q] = a;
   }
}

// ---------------------------------------------------------------- extraction: all A_b as one block-diagonal CSR in extended numbering
// FILL = false: counts; flags bit 0 a row without diagonal entry (bad_dom: the smallest such subdomain)
template <bool FILL>
__global__ __launch_bounds__(256) void k_sw_extract(int next, int n, int V, const int *__restrict__ dom_ptr, const int *__restrict__ dom_rows,
                                                    const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                    int *__restrict__ cnt, const int *__restrict__ orp, int *__restrict__ ocj,
                                                    double *__restrict__ ov, int *flag, int *bad_dom)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p >= next) return;
   const int b = sw_block_of(p, dom_ptr, V), lo = dom_ptr[b], hi = dom_ptr[b + 1], i = dom_rows[p];
   int       c = 0, prev = -1, d = 0, unsorted = 0, o = FILL ? orp[p] : 0;
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int j = cj[k];
      if (j >= n) continue;
      const int q = sw_find(dom_rows, lo, hi, j);
      if (q >= hi || dom_rows[q] != j) continue;
      if (q <= prev) unsorted = 2;
      prev = q;
      d |= (q == p);
      if (FILL) { ocj[o] = q; ov[o] = v[k]; o++; }
      c++;
   }
   if (!FILL)
   {
      cnt[p] = c;
      if (!d) { atomicOr(flag, 1); atomicMin(bad_dom, b); }
      if (unsorted) atomicOr(flag, 2);
   }
}

// ---------------------------------------------------------------- symbolic ILU(k)
// visited table of one row in LDS: open addressing on the vertex id
struct LdsStore {
   int *key, *minm, *st, *lay, *vis, *nf, *fr_v, *fr_m;
   int *nvis, *ovf;
   __device__ __forceinline__ int cap() const { return kCap; }
   __device__ __forceinline__ int keyof(int s) const { return key[s]; }
   __device__ __forceinline__ int slot(int t)
   {
      if (*(volatile int *)ovf) return -1;
      unsigned h = ((unsigned)t * 2654435761u) >> 22; // kHash = 1024 slots
      for (int probe = 0; probe < kHash; probe++, h = (h + 1) & (kHash - 1))
      {
         const int cur = *(volatile int *)&key[h];
         if (cur == t) return (int)h;
         if (cur != -1) continue;
         const int old = atomicCAS(&key[h], -1, t);
         if (old == t) return (int)h;
         if (old != -1) continue;
         const int idx = atomicAdd(nvis, 1);
         if (idx >= kCap) { atomicExch(ovf, 1); return -1; }
         vis[idx] = (int)h;
         return (int)h;
      }
      atomicExch(ovf, 1);
      return -1;
   }
};
static_assert(kHash == 1024, "LdsStore::slot shifts for 1024 slots");
// the same on dense arrays over the row's subdomain [base, base + size) in global memory
struct DenseStore {
   int *minm, *st, *lay, *vis, *nf, *fr_v, *fr_m;
   int *nvis, *ovf;
   int  base, size;
   __device__ __forceinline__ int cap() const { return size; }
   __device__ __forceinline__ int keyof(int s) const { return s + base; }
   __device__ __forceinline__ int slot(int t)
   {
      const int s = t - base;
      if (s < 0 || s >= size) { atomicExch(ovf, 1); return -1; } // (cannot happen: the operator is block-diagonal)
      if (!(atomicOr(&st[s], kSeen) & kSeen))
      {
         const int idx = atomicAdd(nvis, 1);
         if (idx < size) vis[idx] = s;
      }
      return s;
   }
};

// the layered search of row i by one wavefront (64 threads, all of them call); afterwards the entries of the row besides the diagonal
// are the visited slots with kEntry in st.  sh: 4 ints of LDS (visited count, next-frontier count, frontier count, overflow flag)
template <class Store>
__device__ void sw_search(Store &S, int i, int k, const int *__restrict__ rp, const int *__restrict__ cj, int *sh, int tid)
{
   int *nnf = sh + 1, *nfr = sh + 2;
   if (tid == 0)
   {
      sh[0] = 0; sh[1] = 0; sh[2] = 1; sh[3] = 0;
      S.fr_v[0] = i;
      S.fr_m[0] = -1;
   }
   __syncthreads();
   const int g = tid >> 3, l = tid & 7;
   for (int len = 0; len <= k; len++)
   {
      const int nf_now = *nfr;
      for (int f = g; f < nf_now; f += 8)
      {
         const int h = S.fr_v[f];
         const int m2 = (len == 0) ? -1 : max(S.fr_m[f], h); // h becomes an interior vertex
         for (int e = rp[h] + l; e < rp[h + 1]; e += 8)
         {
            const int t = cj[e];
            if (t == i) continue;
            const int s = S.slot(t);
            if (s < 0) continue;
            const int old = atomicMin(&S.minm[s], m2);
            if (m2 >= old) continue;
            if (m2 < t) atomicOr(&S.st[s], kEntry);
            if (t < i && len < k && atomicMax(&S.lay[s], len + 1) < len + 1)
            {
               const int idx = atomicAdd(nnf, 1);
               if (idx < S.cap()) S.nf[idx] = s;
               else atomicExch(S.ovf, 1);
            }
         }
      }
      __syncthreads();
      if (*(volatile int *)S.ovf) return;
      const int nn = *nnf;
      for (int q = tid; q < nn; q += 64)
      { // the next frontier with the m every vertex ended this layer with
         const int s = S.nf[q];
         S.fr_v[q]   = S.keyof(s);
         S.fr_m[q]   = S.minm[s];
      }
      __syncthreads();
      if (tid == 0) { *nfr = nn; *nnf = 0; }
      __syncthreads();
      if (nn == 0) break;
   }
}

// LDS path.  FILL = false: cnt[p] = entries of row p, or -1 for a row that outgrew the table.  FILL = true: the sorted columns of
// the rows that cnt (then the overflow marks) does not flag.
template <bool FILL>
__global__ __launch_bounds__(64) void k_sw_symbolic_lds(int next, int k, const int *__restrict__ rp, const int *__restrict__ cj,
                                                        int *__restrict__ cnt, const int *__restrict__ orp, int *__restrict__ ocj)
{
   __shared__ int key[kHash], minm[kHash], st[kHash], lay[kHash], vis[kCap], nf[kCap + 1], fr_v[kCap], fr_m[kCap], sh[4], total;
   const int      tid = threadIdx.x;
   for (int p = blockIdx.x; p < next; p += gridDim.x)
   {
      if (FILL && orp[p + 1] - orp[p] == 0) continue; // (never: every row has its diagonal)
      if (FILL && cnt[p] != 0) continue;              // (fill pass: cnt holds the overflow marks) the global-memory path writes this row
      for (int q = tid; q < kHash; q += 64) { key[q] = -1; minm[q] = kInf; st[q] = 0; lay[q] = 0; }
      if (tid == 0) total = 0;
      __syncthreads();
      LdsStore S{key, minm, st, lay, vis, nf, fr_v, fr_m, sh, sh + 3};
      sw_search(S, p, k, rp, cj, sh, tid);
      __syncthreads();
      if (sh[3])
      {
         if (!FILL && tid == 0) cnt[p] = -1;
         __syncthreads();
         continue;
      }
      const int nv = sh[0];
      // entries -> nf (the frontier is done with it)
      for (int q = tid; q < nv; q += 64)
         if (st[vis[q]] & kEntry) nf[atomicAdd(&total, 1)] = key[vis[q]];
      __syncthreads();
      if (tid == 0) nf[total] = p; // the diagonal (total <= kCap: nf has one slot more)
      __syncthreads();
      const int m = total + 1;
      if (!FILL)
      {
         if (tid == 0) cnt[p] = m;
      }
      else
      {
         const int o = orp[p];
         for (int q = tid; q < m; q += 64)
         { // rank sort: the columns are distinct
            const int c = nf[q];
            int       r = 0;
            for (int x = 0; x < m; x++) r += (nf[x] < c);
            ocj[o + r] = c;
         }
      }
      __syncthreads();
   }
}

// global-memory path: worker w = blockIdx.x redoes the rows list[w], list[w + W], ... on its own dense arrays (7 x stride ints at ws)
template <bool FILL>
__global__ __launch_bounds__(64) void k_sw_symbolic_dense(int nlist, const int *__restrict__ list, int k, int V, const int *__restrict__ dom_ptr,
                                                          const int *__restrict__ rp, const int *__restrict__ cj, int *__restrict__ ws, int stride,
                                                          int *__restrict__ cnt, const int *__restrict__ orp, int *__restrict__ ocj)
{
   __shared__ int sh[4], total;
   const int      tid = threadIdx.x;
   int           *w0  = ws + (size_t)blockIdx.x * 7 * (size_t)stride;
   for (int li = blockIdx.x; li < nlist; li += gridDim.x)
   {
      const int  p = list[li], b = sw_block_of(p, dom_ptr, V), base = dom_ptr[b], size = dom_ptr[b + 1] - base;
      DenseStore S{w0, w0 + stride, w0 + 2 * (size_t)stride, w0 + 3 * (size_t)stride, w0 + 4 * (size_t)stride, w0 + 5 * (size_t)stride,
                   w0 + 6 * (size_t)stride, sh, sh + 3, base, size};
      if (tid == 0) total = 0;
      __syncthreads();
      sw_search(S, p, k, rp, cj, sh, tid);
      __syncthreads();
      const int nv = min(sh[0], size);
      if (!FILL)
      {
         for (int q = tid; q < nv; q += 64)
            if (S.st[S.vis[q]] & kEntry) atomicAdd(&total, 1);
         __syncthreads();
         if (tid == 0) cnt[p] = total + 1;
      }
      else
      { // ordered sweep over the subdomain: the columns come out sorted
         int o = orp[p];
         for (int c = 0; c < size; c += 64)
         {
            const int  s  = c + tid;
            const bool is = s < size && ((S.st[s] & kEntry) || s + base == p);
            const u64  mk = __ballot(is);
            if (is) ocj[o + __popcll(mk & (((u64)1 << tid) - 1))] = s + base;
            o += __popcll(mk);
         }
      }
      __syncthreads();
      for (int q = tid; q < nv; q += 64)
      { // leave the arrays as they were found
         const int s = S.vis[q];
         S.minm[s]   = kInf;
         S.st[s]     = 0;
         S.lay[s]    = 0;
      }
      __threadfence_block();
      __syncthreads();
   }
}

__global__ __launch_bounds__(256) void k_sw_overflow_mark(int next, const int *__restrict__ cnt, int *__restrict__ mark)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p < next) mark[p] = cnt[p] < 0;
}
__global__ __launch_bounds__(256) void k_sw_overflow_list(int next, const int *__restrict__ pos, int *__restrict__ list)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p < next && pos[p + 1] > pos[p]) list[pos[p]] = p;
}
// the operator's values into the pattern, zeros at the fill positions (both rows column-sorted; the pattern holds the operator's)
__global__ __launch_bounds__(256) void k_sw_scatter(int next, const int *__restrict__ erp, const int *__restrict__ ecj, const double *__restrict__ ev,
                                                    const int *__restrict__ prp, const int *__restrict__ pcj, double *__restrict__ pv,
                                                    int *__restrict__ longest)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p >= next) return;
   int e = erp[p];
   const int ee = erp[p + 1];
   for (int q = prp[p]; q < prp[p + 1]; q++)
   {
      const int c = pcj[q];
      while (e < ee && ecj[e] < c) e++;
      pv[q] = (e < ee && ecj[e] == c) ? ev[e] : 0.0;
   }
   atomicMax(longest, prp[p + 1] - prp[p]);
}
__global__ __launch_bounds__(256) void k_sw_longest(int next, const int *__restrict__ prp, int *__restrict__ longest)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p < next) atomicMax(longest, prp[p + 1] - prp[p]);
}
__global__ __launch_bounds__(256) void k_sw_zero_pivot(int next, const double *__restrict__ v, const int *__restrict__ dg, int *first)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p < next && v[dg[p]] == 0.0) atomicMin(first, p);
}

// ---------------------------------------------------------------- restrict and combine
__global__ __launch_bounds__(256) void k_sw_gather(int next, const int *__restrict__ dom_rows, const double *__restrict__ r, double *__restrict__ re)
{
   const int p = blockIdx.x * 256 + threadIdx.x;
   if (p < next) re[p] = r[dom_rows[p]];
}
__global__ __launch_bounds__(256) void k_sw_ras(int n, double w, const int *__restrict__ own_pos, const double *__restrict__ y, double *__restrict__ z)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) z[i] = w * y[own_pos[i]];
}
__global__ __launch_bounds__(256) void k_sw_as(int n, double w, const int *__restrict__ copy_ptr, const int *__restrict__ copy_pos,
                                               const double *__restrict__ y, double *__restrict__ z)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double s = 0.0;
   for (int c = copy_ptr[i]; c < copy_ptr[i + 1]; c++) s += y[copy_pos[c]];
   z[i] = w * s;
}

void sort_keys(DArray<u64> &keys, DArray<u64> &sorted, size_t m)
{
   size_t tmp_bytes = 0;
   HDA_ROCPRIM(rocprim::radix_sort_keys(nullptr, tmp_bytes, keys.data(), sorted.data(), m, 0, 64, STREAM));
   DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
   HDA_ROCPRIM(rocprim::radix_sort_keys(tmp.data(), tmp_bytes, keys.data(), sorted.data(), m, 0, 64, STREAM));
}
int last_of(const DArray<int> &scan, size_t n)
{
   int t = 0;
   HDA_HIP(hipMemcpyAsync(&t, scan.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   return t;
}
double now_ms()
{
   Context::get().sync();
   return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
const char *kNextMsg = "Schwarz: the extended system (N_ext, the rows of all subdomains together) does not fit int32";

} // namespace

void Schwarz::setup(const DCsr &A, const SchwarzParams &p)
{
   prm = p;
   n   = A.nrows;
   HDA_REQUIRE(p.variant == 0 || p.variant == 1, "Schwarz: variant must be ras-iluk (0) or as-iluk (1)");
   HDA_REQUIRE(p.overlap >= 0 && p.fill >= 0 && p.max_iter >= 1, "Schwarz: overlap >= 0, iluk_level_of_fill >= 0 and max_iter >= 1 are required");
   HDA_REQUIRE(p.fill < 30000, "Schwarz: iluk_level_of_fill is limited to 29999");
   nnz_A = A.nnz;
   // row blocks: the caller's starts, hypre's even split into V, or the setup's own choice (blocks = 0) -- as Ilu::setup
   std::vector<int> bpart;
   {
      int nb = prm.blocks;
      if (nb == 0) nb = amg_auto_blocks(A);
      nb = std::min(std::max(nb, 1), std::max(n, 1));
      if (!prm.block_part.empty())
      {
         HDA_REQUIRE((int)prm.block_part.size() == nb + 1 && prm.block_part.front() == 0 && prm.block_part.back() == n,
                     "Schwarz: block_part must hold blocks + 1 ascending row starts from 0 to the number of rows");
         for (size_t q = 1; q < prm.block_part.size(); q++)
            HDA_REQUIRE(prm.block_part[q] >= prm.block_part[q - 1], "Schwarz: block_part must ascend");
         bpart.assign(prm.block_part.begin(), prm.block_part.end());
      }
      else
      {
         bpart.resize((size_t)nb + 1);
         for (int q = 0; q <= nb; q++) bpart[(size_t)q] = (int)(((__int128)q * n) / nb);
      }
      V = nb;
   }
   HDA_REQUIRE(V < (1 << 30), "Schwarz: too many blocks");
   DArray<int> dpart;
   dpart.upload(bpart.data(), bpart.size());
   const int *rp = A.rowptr.data(), *cj = A.col.data();

   // ---- overlap expansion: one frontier step per layer over (block, row) keys
   double      t0 = now_ms();
   DArray<u64> set((size_t)std::max(n, 1)), front;
   if (n) k_sw_init<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, dpart.data(), V, set.data());
   int nset = n, nfront = n;
   if (prm.overlap > 0 && n)
   {
      front.alloc((size_t)n);
      HDA_HIP(hipMemcpyAsync(front.data(), set.data(), sizeof(u64) * (size_t)n, hipMemcpyDeviceToDevice, STREAM));
   }
   for (int layer = 0; layer < prm.overlap && nfront > 0; layer++)
   {
      DArray<int> cnt((size_t)nfront + 1), off((size_t)nfront + 1);
      cnt.zero();
      k_sw_front_count<<<ceil_div(nfront, 256), 256, 0, STREAM>>>(nfront, front.data(), n, rp, cj, cnt.data());
      require_int32_total(nfront, cnt.data(), "Schwarz overlap candidate list");
      exclusive_scan(nfront, cnt.data(), off.data(), nullptr);
      const int T = last_of(off, (size_t)nfront);
      if (T == 0) break;
      HDA_REQUIRE((long long)nset + T < 2147483647LL, kNextMsg);
      const int   M = nset + T;
      DArray<u64> all((size_t)M), sorted((size_t)M);
      HDA_HIP(hipMemcpyAsync(all.data(), set.data(), sizeof(u64) * (size_t)nset, hipMemcpyDeviceToDevice, STREAM));
      k_sw_front_fill<<<ceil_div(nfront, 256), 256, 0, STREAM>>>(nfront, front.data(), n, rp, cj, off.data(), all.data() + nset);
      sort_keys(all, sorted, (size_t)M);
      DArray<int> head((size_t)M + 1), fresh((size_t)M + 1), hpos((size_t)M + 1), fpos((size_t)M + 1);
      head.zero();
      fresh.zero();
      k_sw_heads<<<ceil_div(M, 256), 256, 0, STREAM>>>(M, sorted.data(), head.data(), fresh.data());
      exclusive_scan(M, head.data(), hpos.data(), nullptr);
      exclusive_scan(M, fresh.data(), fpos.data(), nullptr);
      const int ns = last_of(hpos, (size_t)M), nf = last_of(fpos, (size_t)M);
      DArray<u64> set2((size_t)std::max(ns, 1)), front2((size_t)std::max(nf, 1));
      k_sw_compact<<<ceil_div(M, 256), 256, 0, STREAM>>>(M, sorted.data(), hpos.data(), fpos.data(), set2.data(), front2.data());
      set    = std::move(set2);
      front  = std::move(front2);
      nset   = ns;
      nfront = nf;
   }
   n_ext    = nset;
   identity = (n_ext == n);
   dom_rows.alloc((size_t)std::max(n_ext, 1));
   DArray<int> dom_ptr((size_t)V + 1);
   {
      const int m = std::max(n_ext, V + 1);
      k_sw_dom<<<ceil_div(m, 256), 256, 0, STREAM>>>(n_ext, set.data(), V, dom_rows.data(), dom_ptr.data());
   }
   h_dom_ptr = dom_ptr.to_host();
   own_pos.alloc((size_t)std::max(n, 1));
   copy_ptr.alloc((size_t)n + 1);
   copy_pos.alloc((size_t)std::max(n_ext, 1));
   {
      DArray<u64> keys((size_t)std::max(n_ext, 1)), skeys((size_t)std::max(n_ext, 1));
      const int   m = std::max(n_ext, n + 1);
      if (n_ext) k_sw_inverse<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n, n_ext, dpart.data(), V, dom_ptr.data(), dom_rows.data(), own_pos.data(), keys.data());
      if (n_ext) sort_keys(keys, skeys, (size_t)n_ext);
      k_sw_copies<<<ceil_div(m, 256), 256, 0, STREAM>>>(n, n_ext, skeys.data(), copy_ptr.data(), copy_pos.data());
   }
   set.release();
   front.release();
   double t1 = now_ms();
   setup_ms[0] = t1 - t0;

   // ---- extraction
   DCsr E;
   E.nrows = E.ncols = n_ext;
   E.rowptr.alloc((size_t)n_ext + 1);
   {
      DArray<int> cnt((size_t)n_ext + 1), flag(2);
      cnt.zero();
      const int init[2] = {0, 2147483647};
      flag.upload(init, 2);
      if (n_ext)
         k_sw_extract<false><<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, n, V, dom_ptr.data(), dom_rows.data(), rp, cj, A.val.data(), cnt.data(),
                                                                      nullptr, nullptr, nullptr, flag.data(), flag.data() + 1);
      int f[2];
      flag.download(f, 2);
      if (f[0] & 1)
      {
         char msg[160];
         snprintf(msg, sizeof msg, "Schwarz: a row of subdomain %d has no diagonal entry", f[1]);
         throw Error(msg);
      }
      require_int32_total(n_ext, cnt.data(), "Schwarz subdomain operator");
      exclusive_scan(n_ext, cnt.data(), E.rowptr.data(), nullptr);
      E.nnz = last_of(E.rowptr, (size_t)n_ext);
      E.col.alloc((size_t)std::max(E.nnz, 1));
      E.val.alloc((size_t)std::max(E.nnz, 1));
      if (n_ext)
         k_sw_extract<true><<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, n, V, dom_ptr.data(), dom_rows.data(), rp, cj, A.val.data(), nullptr,
                                                                     E.rowptr.data(), E.col.data(), E.val.data(), nullptr, nullptr);
      if (f[0] & 2) sort_rows(E);
   }
   double t2 = now_ms();
   setup_ms[1] = t2 - t1;

   // ---- symbolic ILU(k): count, scan, fill; rows that outgrow the LDS table on dense arrays in global memory
   DCsr P;
   global_rows = 0;
   if (prm.fill == 0 || n_ext == 0) P = std::move(E); // the input pattern, no search
   else
   {
      const int k = prm.fill;
      P.nrows = P.ncols = n_ext;
      P.rowptr.alloc((size_t)n_ext + 1);
      DArray<int> cnt((size_t)n_ext + 1), mark((size_t)n_ext + 1), pos((size_t)n_ext + 1), list, ws;
      cnt.zero();
      mark.zero();
      const int grid = std::min(n_ext, 8192);
      k_sw_symbolic_lds<false><<<grid, 64, 0, STREAM>>>(n_ext, k, E.rowptr.data(), E.col.data(), cnt.data(), nullptr, nullptr);
      k_sw_overflow_mark<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, cnt.data(), mark.data());
      exclusive_scan(n_ext, mark.data(), pos.data(), nullptr);
      global_rows = last_of(pos, (size_t)n_ext);
      int workers = 0, stride = 0;
      if (global_rows)
      {
         for (int b = 0; b < V; b++) stride = std::max(stride, h_dom_ptr[(size_t)b + 1] - h_dom_ptr[(size_t)b]);
         workers = std::min(global_rows, kWorkers);
         list.alloc((size_t)global_rows);
         ws.alloc((size_t)workers * 7 * (size_t)stride);
         HDA_HIP(hipMemsetAsync(ws.data(), 0, ws.size() * sizeof(int), STREAM));
         for (int w = 0; w < workers; w++) // minm = "no path yet"
            HDA_HIP(hipMemsetAsync(ws.data() + (size_t)w * 7 * (size_t)stride, 0x7f, (size_t)stride * sizeof(int), STREAM));
         k_sw_overflow_list<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, pos.data(), list.data());
         k_sw_symbolic_dense<false><<<workers, 64, 0, STREAM>>>(global_rows, list.data(), k, V, dom_ptr.data(), E.rowptr.data(), E.col.data(),
                                                               ws.data(), stride, cnt.data(), nullptr, nullptr);
      }
      require_int32_total(n_ext, cnt.data(), "Schwarz ILU(k) factor");
      exclusive_scan(n_ext, cnt.data(), P.rowptr.data(), nullptr);
      P.nnz = last_of(P.rowptr, (size_t)n_ext);
      P.col.alloc((size_t)std::max(P.nnz, 1));
      P.val.alloc((size_t)std::max(P.nnz, 1));
      if (global_rows)
      { // (the fill pass of the LDS kernel skips the marked rows)
         k_sw_symbolic_dense<true><<<workers, 64, 0, STREAM>>>(global_rows, list.data(), k, V, dom_ptr.data(), E.rowptr.data(), E.col.data(),
                                                              ws.data(), stride, nullptr, P.rowptr.data(), P.col.data());
      }
      k_sw_symbolic_lds<true><<<grid, 64, 0, STREAM>>>(n_ext, k, E.rowptr.data(), E.col.data(), mark.data(), P.rowptr.data(), P.col.data());
   }
   double t3 = now_ms();
   setup_ms[2] = t3 - t2;

   // ---- numeric factorisation on the pattern (hda_ilu.hip), substitutions block-parallel over the subdomains
   {
      DArray<int> longest(1);
      longest.zero();
      if (prm.fill > 0 && n_ext)
      {
         k_sw_scatter<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, E.rowptr.data(), E.col.data(), E.val.data(), P.rowptr.data(), P.col.data(),
                                                               P.val.data(), longest.data());
      }
      else if (n_ext) k_sw_longest<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, P.rowptr.data(), longest.data());
      longest.download(&longest_row, 1);
      E = DCsr();
      IluParams ip;
      ip.tri_solve = 1;
      ip.max_iter  = 1;
      ip.blocks    = V;
      const int f  = F.setup_pattern(std::move(P), ip, h_dom_ptr);
      if (f & 4)
      {
         DArray<int> first(1);
         const int   big = 2147483647;
         first.upload(&big, 1);
         k_sw_zero_pivot<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, F.factors().val.data(), F.diag_pos(), first.data());
         int row = 0;
         first.download(&row, 1);
         const int b = (int)(std::upper_bound(h_dom_ptr.begin(), h_dom_ptr.end(), row) - h_dom_ptr.begin()) - 1;
         char      msg[160];
         snprintf(msg, sizeof msg, "Schwarz: zero pivot in the ILU(%d) factorisation of subdomain %d", prm.fill, b);
         throw Error(msg);
      }
   }
   r_ext.alloc((size_t)std::max(n_ext, 1));
   y_ext.alloc((size_t)std::max(n_ext, 1));
   setup_ms[3] = now_ms() - t3;
}

// z = M^-1 r: gather, all subdomain solves at once, combine (r and z may not alias)
void Schwarz::apply(const double *r, double *z)
{
   if (n == 0) return;
   if (identity && prm.weight == 1.0)
   { // no overlap: the extended vectors are the caller's, both variants are the plain block solve
      F.apply(r, z);
      return;
   }
   const double *re = r;
   if (!identity)
   {
      k_sw_gather<<<ceil_div(n_ext, 256), 256, 0, STREAM>>>(n_ext, dom_rows.data(), r, r_ext.data());
      re = r_ext.data();
   }
   F.apply(re, y_ext.data());
   if (prm.variant == 0) k_sw_ras<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, prm.weight, own_pos.data(), y_ext.data(), z);
   else k_sw_as<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, prm.weight, copy_ptr.data(), copy_pos.data(), y_ext.data(), z);
}

} // namespace hda
