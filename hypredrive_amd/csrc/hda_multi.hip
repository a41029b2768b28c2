// hda_multi.hip -- up to 8 right-hand sides at once (hda_multi.h): SpMM on the plain CSR arrays, batched BLAS-1,
// the batched V-cycle (Amg::apply_multi) and k PCG recurrences in lockstep (pcg_multi).
//
// Every kernel on the solve path is bound by HBM, and the matrix is most of the bytes: with K vectors carried through one pass the
// (col, val) stream -- 12 B per entry -- is paid once for all of them, and the gather of x[col] becomes one contiguous read of 8 K
// bytes.  Nothing here reads the coded, row-class or windowed shadows of an operator, so the path serves a general matrix.
#include "hda_multi.h"

#include "hda_comm.h"

#include <cmath>

namespace hda {

#define STREAM (Context::get().stream)

std::string multi_refusal(int k)
{
   if (k < 1) return "k: at least one right-hand side is required (k >= 1)";
   if (k > kMultiMax) return "k: at most 8 right-hand sides are solved at once (k <= 8)";
   if (Comm::world().size > 1) return "more than one rank: the batched solve is built on one rank";
   return std::string();
}

MultiScratch &MultiScratch::get()
{
   MultiScratch &s = RankState<MultiScratch, 23>::get();
   if (!s.host_scalars)
   {
      s.partials.alloc((size_t)kMultiSlots * kMultiMax * kRedBlocks);
      s.scalars.alloc((size_t)kMultiScalars * kMultiMax);
      s.active.alloc(kMultiMax);
      s.partials.zero();
      s.scalars.zero();
      s.active.zero();
      HDA_HIP(hipHostMalloc((void **)&s.host_scalars, sizeof(double) * kMultiScalars * kMultiMax));
      HDA_HIP(hipHostMalloc((void **)&s.host_active, sizeof(int) * kMultiMax));
      for (int q = 0; q < kMultiScalars * kMultiMax; q++) s.host_scalars[q] = 0.0;
      for (int j = 0; j < kMultiMax; j++) s.host_active[j] = 0;
   }
   return s;
}

// ------------------------------------------------------- device helpers

namespace {

// (the reductions of hda_kernels.hip, restated: a batched dot product takes the tree of dot() so that a column's sum has the bits the
// single kernel gives it)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}
__device__ __forceinline__ double block_sum(double v)
{
   __shared__ double sm[4];
   v = wave_sum(v);
   if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
   __syncthreads();
   double t = (sm[0] + sm[1]) + (sm[2] + sm[3]);
   __syncthreads();
   return t;
}
template <int L>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
   for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}
__device__ __forceinline__ double slot_sum_256(const double *__restrict__ p)
{
   double s = 0.0;
   for (int i = threadIdx.x; i < kRedBlocks; i += kRedThreads) s += p[i];
   return block_sum(s);
}

// one row of an interleaved vector: K doubles, 16 B at a time (rows start on a multiple of 16 B: K >= 2, arrays from the allocator)
template <int K>
__device__ __forceinline__ void load_row(const double *__restrict__ p, double (&v)[K])
{
   const double2 *q = reinterpret_cast<const double2 *>(p);
#pragma unroll
   for (int h = 0; h < K / 2; h++)
   {
      const double2 t = q[h];
      v[2 * h]        = t.x;
      v[2 * h + 1]    = t.y;
   }
}
template <int K>
__device__ __forceinline__ void store_row(double *__restrict__ p, const double (&v)[K])
{
   double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
   for (int h = 0; h < K / 2; h++) q[h] = make_double2(v[2 * h], v[2 * h + 1]);
}

inline int ew_grid(long n) { return (int)std::min<long>(std::max<long>((n + 255) / 256, 1), kRedBlocks); }

template <class F>
void for_width(int K, F &&f)
{
   if (K == 2) f(std::integral_constant<int, 2>());
   else if (K == 4) f(std::integral_constant<int, 4>());
   else if (K == 8) f(std::integral_constant<int, 8>());
   else throw Error("batched kernels: the storage width K must be 2, 4 or 8");
}

} // namespace

// ------------------------------------------------------- layout

template <int K>
__global__ __launch_bounds__(256) void k_mpack(int n, int k, const double *__restrict__ src, long long ld, double *__restrict__ dst)
{
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      double v[K];
#pragma unroll
      for (int j = 0; j < K; j++) v[j] = j < k ? src[(size_t)j * (size_t)ld + (size_t)i] : 0.0;
      store_row<K>(dst + (size_t)i * K, v);
   }
}
template <int K>
__global__ __launch_bounds__(256) void k_munpack(int n, int k, const double *__restrict__ src, double *__restrict__ dst, long long ld)
{
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      double v[K];
      load_row<K>(src + (size_t)i * K, v);
#pragma unroll
      for (int j = 0; j < K; j++)
         if (j < k) dst[(size_t)j * (size_t)ld + (size_t)i] = v[j];
   }
}
template <int K>
__global__ __launch_bounds__(256) void k_mcopy_columns(int n, unsigned mask, const double *__restrict__ X, double *__restrict__ Y)
{
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
#pragma unroll
      for (int j = 0; j < K; j++)
         if (mask >> j & 1u) Y[(size_t)i * K + j] = X[(size_t)i * K + j];
}
template <int K>
__global__ __launch_bounds__(256) void k_mscale(int n, const double *__restrict__ d, const double *__restrict__ R, double *__restrict__ Z)
{
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      double       v[K];
      const double di = d[i];
      load_row<K>(R + (size_t)i * K, v);
#pragma unroll
      for (int j = 0; j < K; j++) v[j] = di * v[j];
      store_row<K>(Z + (size_t)i * K, v);
   }
}

void multi_pack(int n, int k, int K, const double *src, long long ld, double *dst)
{
   if (n > 0) for_width(K, [&](auto W) { k_mpack<decltype(W)::value><<<ew_grid(n), 256, 0, STREAM>>>(n, k, src, ld, dst); });
}
void multi_unpack(int n, int k, int K, const double *src, double *dst, long long ld)
{
   if (n > 0) for_width(K, [&](auto W) { k_munpack<decltype(W)::value><<<ew_grid(n), 256, 0, STREAM>>>(n, k, src, dst, ld); });
}
void multi_copy(int n, int K, const double *X, double *Y) { copy(n * K, X, Y); }
void multi_zero(int n, int K, double *X) { fill(n * K, 0.0, X); }
void multi_copy_columns(int n, int K, unsigned mask, const double *X, double *Y)
{
   if (n > 0 && mask) for_width(K, [&](auto W) { k_mcopy_columns<decltype(W)::value><<<ew_grid(n), 256, 0, STREAM>>>(n, mask, X, Y); });
}
void multi_scale(int n, int K, const double *d, const double *R, double *Z)
{
   if (n > 0) for_width(K, [&](auto W) { k_mscale<decltype(W)::value><<<ew_grid(n), 256, 0, STREAM>>>(n, d, R, Z); });
}

// ------------------------------------------------------- SpMM

// lane classes: rows of at most 8, 16, 32, 64 entries share 4, 8, 16, 32 lanes (at most two passes of the row's lanes), longer rows
// a wavefront.  The class is a function of the row's length alone, so the order in which a row's products are summed is too.
__device__ __forceinline__ int mm_class(int len) { return len <= 8 ? 0 : len <= 16 ? 1 : len <= 32 ? 2 : len <= 64 ? 3 : 4; }

__global__ __launch_bounds__(256) void k_mm_class_flag(int n, const int *__restrict__ rp, int cls, int *__restrict__ flag)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) flag[i] = mm_class(rp[i + 1] - rp[i]) == cls;
}
__global__ __launch_bounds__(256) void k_mm_class_fill(int n, const int *__restrict__ flag, const int *__restrict__ pos, int base, int *__restrict__ rows)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && flag[i]) rows[base + pos[i]] = i;
}

static void ensure_row_classes(const DCsr &A)
{
   if (A.mrows_gen == A.gen && A.mrows.size() >= (size_t)A.nrows) return;
   const int   n = A.nrows;
   DArray<int> flag((size_t)n), pos((size_t)n + 1);
   A.mrows.alloc((size_t)n);
   A.mrow_off[0] = 0;
   for (int c = 0; c < 5; c++)
   {
      k_mm_class_flag<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), c, flag.data());
      exclusive_scan(n, flag.data(), pos.data(), nullptr);
      int count = 0;
      download_sync(&count, pos.data() + n, sizeof(int));
      HDA_REQUIRE(count >= 0 && A.mrow_off[c] + count <= n, "row classes of the batched product do not add up");
      if (count) k_mm_class_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, flag.data(), pos.data(), A.mrow_off[c], A.mrows.data());
      A.mrow_off[c + 1] = A.mrow_off[c] + count;
   }
   HDA_REQUIRE(A.mrow_off[5] == n, "row classes of the batched product do not cover the rows");
   A.mrows_gen = A.gen;
}

struct MmPlan {
   const int *rows;
   int        row_off[6];  // class c: rows[row_off[c] .. row_off[c + 1])
   int        tile_off[6]; // ... worked on by the tiles [tile_off[c], tile_off[c + 1]); a tile = the 64 / L rows one wavefront holds
};

// one tile: 64 / L rows of the L-lane class, lane t of a row's group takes the entries t, t + L, ... in order; K accumulators per lane
template <int L, int K, int MODE, bool DOT>
__device__ __forceinline__ void mm_tile(int first, int count, const int *__restrict__ rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                        const double *__restrict__ val, const double *__restrict__ X, double alpha, double beta, const double *Yin,
                                        const double *__restrict__ B, const double *__restrict__ d, const double *__restrict__ W, double *Out,
                                        double (&dacc)[K])
{
   const int  lane = threadIdx.x & 63, t = lane & (L - 1);
   const int  idx  = first + lane / L;
   const bool has  = idx < count;
   int        r = 0, s = 0, e = 0;
   if (has)
   {
      r = rows[idx];
      s = rowptr[r];
      e = rowptr[r + 1];
   }
   double acc[K];
#pragma unroll
   for (int j = 0; j < K; j++) acc[j] = 0.0;
   for (int q = s + t; q < e; q += L) // (a row longer than one pass of its lanes loops)
   {
      const double v = val[q];
      double       xv[K];
      load_row<K>(X + (size_t)col[q] * K, xv);
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] += v * xv[j];
   }
#pragma unroll
   for (int j = 0; j < K; j++) acc[j] = group_sum<L>(acc[j]); // (every lane of the wavefront takes part: rows past the end sum zeros)
   if (has && t == 0)
   {
      const size_t o = (size_t)r * K;
      double       out[K], aux[K];
      if (MODE == MM_PLAIN)
      {
         if (beta == 0.0)
         {
#pragma unroll
            for (int j = 0; j < K; j++) out[j] = alpha * acc[j];
         }
         else
         {
            load_row<K>(Yin + o, aux);
#pragma unroll
            for (int j = 0; j < K; j++) out[j] = alpha * acc[j] + beta * aux[j];
         }
      }
      else if (MODE == MM_RESID)
      {
         load_row<K>(B + o, aux);
#pragma unroll
         for (int j = 0; j < K; j++) out[j] = aux[j] - acc[j];
      }
      else
      {
         double       xr[K];
         const double di = d[r];
         load_row<K>(B + o, aux);
         load_row<K>(X + o, xr);
#pragma unroll
         for (int j = 0; j < K; j++) out[j] = xr[j] + di * (aux[j] - acc[j]);
      }
      if (DOT)
      {
         load_row<K>(W + o, aux);
#pragma unroll
         for (int j = 0; j < K; j++) dacc[j] += aux[j] * out[j];
      }
      store_row<K>(Out + o, out);
   }
}

// Tiles are dealt to the wavefronts of the grid round robin; which class a tile belongs to is wavefront-uniform.  DOT: the grid is
// kRedBlocks blocks and block b leaves the partial of column j at partial[j * kRedBlocks + b] (no atomics: a run repeats bit for bit).
template <int K, int MODE, bool DOT>
__global__ __launch_bounds__(256) void k_spmm(MmPlan pl, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                                              const double *__restrict__ X, double alpha, double beta, const double *Yin, const double *__restrict__ B,
                                              const double *__restrict__ d, const double *__restrict__ W, double *Out, double *__restrict__ partial)
{
   double dacc[K];
#pragma unroll
   for (int j = 0; j < K; j++) dacc[j] = 0.0;
   const int T = pl.tile_off[5];
   for (long tl = (long)blockIdx.x * 4 + (threadIdx.x >> 6); tl < T; tl += (long)gridDim.x * 4)
   {
      const int tile = __builtin_amdgcn_readfirstlane((int)tl);
#define HDA_MM_TILE(c, L)                                                                                                          \
   mm_tile<L, K, MODE, DOT>((tile - pl.tile_off[c]) * (64 / L), pl.row_off[c + 1] - pl.row_off[c], pl.rows + pl.row_off[c], rowptr, col, val, \
                            X, alpha, beta, Yin, B, d, W, Out, dacc)
      if (tile < pl.tile_off[1]) HDA_MM_TILE(0, 4);
      else if (tile < pl.tile_off[2]) HDA_MM_TILE(1, 8);
      else if (tile < pl.tile_off[3]) HDA_MM_TILE(2, 16);
      else if (tile < pl.tile_off[4]) HDA_MM_TILE(3, 32);
      else HDA_MM_TILE(4, 64);
#undef HDA_MM_TILE
   }
   if (DOT)
   {
#pragma unroll
      for (int j = 0; j < K; j++)
      {
         const double s = block_sum(dacc[j]);
         if (threadIdx.x == 0) partial[(size_t)j * kRedBlocks + blockIdx.x] = s;
      }
   }
}

template <int K, int MODE, bool DOT>
static void launch_spmm(const MmPlan &pl, const DCsr &A, double alpha, const double *X, double beta, const double *Yin, const double *B, const double *d,
                        const double *W, double *Out, double *partial)
{
   const int grid = DOT ? kRedBlocks : ceil_div(pl.tile_off[5], 4);
   k_spmm<K, MODE, DOT><<<grid, 256, 0, STREAM>>>(pl, A.rowptr.data(), A.col.data(), A.val.data(), X, alpha, beta, Yin, B, d, W, Out, partial);
}

void spmm(const DCsr &A, int K, int mode, double alpha, const double *X, double beta, const double *Yin, const double *B, const double *d,
          const double *W, double *Out, int dot_slot)
{
   if (A.nrows == 0) return;
   HDA_REQUIRE(mode == MM_PLAIN || mode == MM_RESID || mode == MM_JACOBI, "spmm: unknown mode");
   HDA_REQUIRE(mode != MM_JACOBI || Out != X, "spmm: the Jacobi sweep is out of place");
   HDA_REQUIRE((W != nullptr) == (dot_slot >= 0) && dot_slot < kMultiSlots, "spmm: a dot product needs W and a slot");
   ensure_row_classes(A);
   MmPlan pl;
   pl.rows        = A.mrows.data();
   pl.tile_off[0] = 0;
   for (int c = 0; c < 5; c++)
   {
      pl.row_off[c]      = A.mrow_off[c];
      const int per      = 64 / (4 << c);
      pl.tile_off[c + 1] = pl.tile_off[c] + ceil_div(A.mrow_off[c + 1] - A.mrow_off[c], per);
   }
   pl.row_off[5] = A.mrow_off[5];
   double *partial = dot_slot >= 0 ? MultiScratch::get().slot(dot_slot) : nullptr;
   for_width(K, [&](auto Wd) {
      constexpr int KK = decltype(Wd)::value;
      if (mode == MM_PLAIN)
      {
         if (W) launch_spmm<KK, MM_PLAIN, true>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
         else launch_spmm<KK, MM_PLAIN, false>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
      }
      else if (mode == MM_RESID)
      {
         if (W) launch_spmm<KK, MM_RESID, true>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
         else launch_spmm<KK, MM_RESID, false>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
      }
      else
      {
         if (W) launch_spmm<KK, MM_JACOBI, true>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
         else launch_spmm<KK, MM_JACOBI, false>(pl, A, alpha, X, beta, Yin, B, d, W, Out, partial);
      }
   });
}

double spmm_bytes(const DCsr &A, int K, int mode, bool dot)
{
   const double n     = A.nrows;
   const int    extra = (mode == MM_PLAIN ? 0 : 1) + (dot ? 1 : 0); // b (the sweep's own x rows come with the gather), w
   return 12.0 * A.nnz + 4.0 * (n + 1.0) + 8.0 * K * A.ncols + 8.0 * K * n + 8.0 * K * n * extra;
}

// ------------------------------------------------------- batched BLAS-1

// thread -> rows as k_dot deals them, one accumulator per column, the block tree of dot(): column j alone through dot() has these bits
template <int K>
__global__ __launch_bounds__(256) void k_mdot(int n, const double *__restrict__ X, const double *__restrict__ Y, double *__restrict__ partial)
{
   double acc[K];
#pragma unroll
   for (int j = 0; j < K; j++) acc[j] = 0.0;
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      double x[K], y[K];
      load_row<K>(X + (size_t)i * K, x);
      load_row<K>(Y + (size_t)i * K, y);
#pragma unroll
      for (int j = 0; j < K; j++) acc[j] += x[j] * y[j];
   }
#pragma unroll
   for (int j = 0; j < K; j++)
   {
      const double s = block_sum(acc[j]);
      if (threadIdx.x == 0) partial[(size_t)j * kRedBlocks + blockIdx.x] = s;
   }
}
void multi_dot(int n, int K, const double *X, const double *Y, int slot)
{
   double *p = MultiScratch::get().slot(slot);
   for_width(K, [&](auto W) { k_mdot<decltype(W)::value><<<kRedBlocks, 256, 0, STREAM>>>(n, X, Y, p); });
}

// block (j, s): scalar block (first_block + s), column j = sum of slot (first_slot + s), column j -- the arithmetic of k_finalize
__global__ __launch_bounds__(kRedThreads) void k_mfinalize(const double *__restrict__ partials, int first_slot, double *__restrict__ scalars, int first_block)
{
   const int    j = blockIdx.x, s = blockIdx.y;
   const double v = slot_sum_256(partials + ((size_t)(first_slot + s) * kMultiMax + j) * kRedBlocks);
   if (threadIdx.x == 0) scalars[(size_t)(first_block + s) * kMultiMax + j] = v;
}
void multi_finalize(int K, int first_slot, int nslots, int first_block)
{
   MultiScratch &m = MultiScratch::get();
   k_mfinalize<<<dim3(K, nslots), kRedThreads, 0, STREAM>>>(m.partials.data(), first_slot, m.scalars.data(), first_block);
}

__global__ __launch_bounds__(kRedThreads) void k_mcg_alpha(const double *__restrict__ partials, double *__restrict__ scalars, const int *__restrict__ active,
                                                           int go)
{
   const int    j  = blockIdx.x;
   const double sp = slot_sum_256(partials + ((size_t)MS_SP * kMultiMax + j) * kRedBlocks);
   if (threadIdx.x == 0)
   {
      scalars[MV_SP * kMultiMax + j]    = sp;
      const bool ok                     = active[j] && sp != 0.0 && isfinite(sp);
      scalars[MV_ALPHA * kMultiMax + j] = ok ? scalars[go * kMultiMax + j] / sp : 0.0;
   }
}
void multi_cg_alpha(int K, int gamma_block)
{
   MultiScratch &m = MultiScratch::get();
   k_mcg_alpha<<<K, kRedThreads, 0, STREAM>>>(m.partials.data(), m.scalars.data(), m.active.data(), gamma_block);
}
__global__ __launch_bounds__(kRedThreads) void k_mcg_beta(const double *__restrict__ partials, double *__restrict__ scalars, const int *__restrict__ active,
                                                          int go, int gn)
{
   const int    j  = blockIdx.x;
   const double g  = slot_sum_256(partials + ((size_t)MS_GAMMA * kMultiMax + j) * kRedBlocks);
   const double rr = slot_sum_256(partials + ((size_t)MS_RR * kMultiMax + j) * kRedBlocks);
   if (threadIdx.x == 0)
   {
      scalars[gn * kMultiMax + j]       = g;
      scalars[(gn + 1) * kMultiMax + j] = rr;
      const bool ok                     = active[j] && scalars[MV_ALPHA * kMultiMax + j] != 0.0;
      scalars[MV_BETA * kMultiMax + j]  = ok ? g / scalars[go * kMultiMax + j] : 0.0;
   }
}
void multi_cg_beta(int K, int gamma_old_block, int gamma_new_block)
{
   MultiScratch &m = MultiScratch::get();
   k_mcg_beta<<<K, kRedThreads, 0, STREAM>>>(m.partials.data(), m.scalars.data(), m.active.data(), gamma_old_block, gamma_new_block);
}

// rows dealt as k_cg_update deals them; a column with alpha_j == 0 is not written (x + 0 p would turn a -0.0 into +0.0)
template <int K>
__global__ __launch_bounds__(256) void k_mcg_update(int n, const double *__restrict__ alpha, const double *__restrict__ P, const double *__restrict__ S,
                                                    double *__restrict__ X, double *__restrict__ R, double *__restrict__ partial)
{
   double a[K], acc[K];
#pragma unroll
   for (int j = 0; j < K; j++)
   {
      a[j]   = alpha[j];
      acc[j] = 0.0;
   }
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      const size_t o = (size_t)i * K;
      double       p[K], s[K], x[K], r[K];
      load_row<K>(P + o, p);
      load_row<K>(S + o, s);
      load_row<K>(X + o, x);
      load_row<K>(R + o, r);
#pragma unroll
      for (int j = 0; j < K; j++)
      {
         if (a[j] != 0.0)
         {
            x[j] += a[j] * p[j];
            r[j] = r[j] - a[j] * s[j];
         }
         acc[j] += r[j] * r[j];
      }
      store_row<K>(X + o, x);
      store_row<K>(R + o, r);
   }
#pragma unroll
   for (int j = 0; j < K; j++)
   {
      const double t = block_sum(acc[j]);
      if (threadIdx.x == 0) partial[(size_t)j * kRedBlocks + blockIdx.x] = t;
   }
}
void multi_cg_update(int n, int K, const double *alpha, const double *P, const double *S, double *X, double *R, int rr_slot)
{
   double *p = MultiScratch::get().slot(rr_slot);
   for_width(K, [&](auto W) { k_mcg_update<decltype(W)::value><<<kRedBlocks, 256, 0, STREAM>>>(n, alpha, P, S, X, R, p); });
}
template <int K>
__global__ __launch_bounds__(256) void k_mcg_dir(int n, const double *__restrict__ beta, const double *__restrict__ Z, double *__restrict__ P)
{
   double b[K];
#pragma unroll
   for (int j = 0; j < K; j++) b[j] = beta[j];
   for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
   {
      const size_t o = (size_t)i * K;
      double       z[K], p[K];
      load_row<K>(Z + o, z);
      load_row<K>(P + o, p);
#pragma unroll
      for (int j = 0; j < K; j++) p[j] = z[j] + b[j] * p[j];
      store_row<K>(P + o, p);
   }
}
void multi_cg_dir(int n, int K, const double *beta, const double *Z, double *P)
{
   if (n > 0) for_width(K, [&](auto W) { k_mcg_dir<decltype(W)::value><<<ew_grid(n), 256, 0, STREAM>>>(n, beta, Z, P); });
}

__global__ void k_mmask(int K, const double *__restrict__ in, const int *__restrict__ active, double *__restrict__ out)
{
   const int j = threadIdx.x;
   if (j < K) out[j] = active[j] ? in[j] : 0.0;
}
void multi_masked(int K, const double *in, int block)
{
   MultiScratch &m = MultiScratch::get();
   k_mmask<<<1, 64, 0, STREAM>>>(K, in, m.active.data(), m.block(block));
}

void multi_set_active(const int *flags)
{
   MultiScratch &m = MultiScratch::get();
   Context::get().sync(); // (the pinned source may still be read by an earlier copy)
   for (int j = 0; j < kMultiMax; j++) m.host_active[j] = flags[j];
   HDA_HIP(hipMemcpyAsync(m.active.data(), m.host_active, sizeof(int) * kMultiMax, hipMemcpyHostToDevice, STREAM));
}
void multi_read_scalars_async(int first_block, int nblocks)
{
   MultiScratch &m = MultiScratch::get();
   Context      &c = Context::get();
   HDA_HIP(hipMemcpyAsync(m.host_scalars + (size_t)first_block * kMultiMax, m.scalars.data() + (size_t)first_block * kMultiMax,
                          sizeof(double) * kMultiMax * (size_t)nblocks, hipMemcpyDeviceToHost, c.stream));
   HDA_HIP(hipEventRecord(c.ev, c.stream));
}

// ------------------------------------------------------- dense coarse solve

// thread i: row i of the inverse against the K columns of F, the terms in the order of k_dense_apply.  F is read by every thread at
// the same address (a broadcast); the level is latency bound as the single solve is
template <int K>
__global__ __launch_bounds__(256) void k_mdense_apply(int n, const double *__restrict__ invT, const double *__restrict__ F, double *__restrict__ X)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double s[K];
#pragma unroll
   for (int j = 0; j < K; j++) s[j] = 0.0;
   for (int m = 0; m < n; m++)
   {
      const double a = invT[(size_t)m * n + i];
      double       f[K];
      load_row<K>(F + (size_t)m * K, f);
#pragma unroll
      for (int j = 0; j < K; j++) s[j] += a * f[j];
   }
   store_row<K>(X + (size_t)i * K, s);
}
void multi_dense_apply(int n, int K, const double *invT, const double *F, double *X)
{
   if (n > 0) for_width(K, [&](auto W) { k_mdense_apply<decltype(W)::value><<<ceil_div(n, 256), 256, 0, STREAM>>>(n, invT, F, X); });
}

// ------------------------------------------------------- batched V-cycle

std::string Amg::multi_cycle_refusal() const
{
   if (dist || tail || Comm::world().size > 1) return "more than one rank: the batched V-cycle is built on one rank";
   if (blocks_used != 1) return "blocks: the batched V-cycle is built for one row block (blocks: 1)";
   for (const AmgLevel &lv : levels)
   {
      if (lv.ilu) return "smoother.type ilu: the batched V-cycle has no ILU smoother";
      if (lv.fsai) return "smoother.type fsai: the batched V-cycle has no FSAI smoother";
      if (lv.gs.nblk > 0 || !lv.blk_part.empty()) return "blocks: the batched V-cycle is built for one row block (blocks: 1)";
   }
   const int L = num_levels();
   for (int dir = 0; dir < 2; dir++)
   {
      const int   t     = dir == 0 ? prm.relax_down : prm.relax_up;
      const char *where = dir == 0 ? "relaxation.down_type" : "relaxation.up_type";
      if (L > 1 && (dir == 0 ? prm.sweeps_down : prm.sweeps_up) > 0 && !is_jacobi_type(t))
      {
         const char *what = is_gs_type(t) ? "hybrid Gauss-Seidel" : is_two_stage_type(t) ? "two-stage Gauss-Seidel" : t == 16 ? "Chebyshev" : "this smoother";
         return std::string(where) + " " + std::to_string(t) + " (" + what + "): the batched V-cycle runs the Jacobi family (0, 7, 18) only";
      }
   }
   if (L > 1 && needs_cf_in_cycle()) return "relaxation.points: F- and C-point sweeps (air) are not built in the batched V-cycle, only points: all";
   if (!coarse_dense && !(prm.relax_coarse == 9 || is_jacobi_type(prm.relax_coarse)))
   {
      const int   t    = prm.relax_coarse;
      const char *what = is_gs_type(t) ? "hybrid Gauss-Seidel" : is_two_stage_type(t) ? "two-stage Gauss-Seidel" : t == 16 ? "Chebyshev" : "this smoother";
      return "relaxation.coarse_type " + std::to_string(t) + " (" + what + "): the batched V-cycle solves the coarsest level with ge (9) or Jacobi sweeps";
   }
   return std::string();
}

void Amg::apply_multi(const double *B, double *X, int K)
{
   HDA_REQUIRE(K == 2 || K == 4 || K == 8, "apply_multi: the storage width K must be 2, 4 or 8");
   const std::string why = multi_cycle_refusal();
   if (!why.empty()) throw Error(why);
   const int L = num_levels();
   if (multi_K_ != K || (int)multi_work_.size() != L)
   {
      multi_work_.clear();
      multi_work_.resize((size_t)L);
      multi_K_ = K;
   }
   for (int l = 0; l < L; l++)
   {
      const size_t need = (size_t)std::max(level_A(l).nrows, 1) * K;
      MultiWork   &w    = multi_work_[(size_t)l];
      if (w.u2.size() != need)
      {
         w.u2.alloc(need);
         w.t.alloc(need);
         if (l > 0) { w.f.alloc(need); w.u.alloc(need); }
      }
   }
   // Jacobi sweeps of one level: the first from a zero guess is the scale kernel; the last lands in `cur`
   auto sweeps = [&](int l, int dir, int count, bool zero, const double *f, double *&cur, double *&alt) {
      const DCsr &A = level_A(l);
      if (zero && count == 0) multi_zero(A.nrows, K, cur);
      for (int s = 0; s < count; s++)
      {
         const double *d = (l == L - 1) ? levels[(size_t)l].dinv_down.data() : sweep_dinv(l, dir, s);
         if (zero && s == 0) multi_scale(A.nrows, K, d, f, cur);
         else
         {
            spmm(A, K, MM_JACOBI, 1.0, cur, 0.0, nullptr, f, d, nullptr, alt, -1);
            std::swap(cur, alt);
         }
      }
   };
   auto coarsest = [&](const double *f, double *&cur, double *&alt) {
      if (coarse_dense) multi_dense_apply(coarse_n, K, coarse_invT.data(), f, cur);
      else sweeps(L - 1, 0, std::max(prm.sweeps_coarse, 1), true, f, cur, alt);
   };
   if (L == 1)
   {
      double *cur = X, *alt = multi_work_[0].u2.data();
      coarsest(B, cur, alt);
      if (cur != X) multi_copy(level_A(0).nrows, K, cur, X);
      return;
   }
   std::vector<double *> sol((size_t)L, nullptr), spare((size_t)L, nullptr);
   const double         *f = B;
   for (int l = 0; l < L - 1; l++)
   {
      MultiWork &w   = multi_work_[(size_t)l];
      double    *cur = l == 0 ? X : w.u.data(), *alt = w.u2.data();
      sweeps(l, 0, prm.sweeps_down, true, f, cur, alt);
      spmm(level_A(l), K, MM_RESID, 1.0, cur, 0.0, nullptr, f, nullptr, nullptr, w.t.data(), -1);
      MultiWork &nx = multi_work_[(size_t)l + 1];
      spmm(levels[(size_t)l].R, K, MM_PLAIN, 1.0, w.t.data(), 0.0, nullptr, nullptr, nullptr, nullptr, nx.f.data(), -1);
      sol[(size_t)l]   = cur;
      spare[(size_t)l] = alt;
      f                = nx.f.data();
   }
   {
      MultiWork &w   = multi_work_[(size_t)L - 1];
      double    *cur = w.u.data(), *alt = w.u2.data();
      coarsest(w.f.data(), cur, alt);
      sol[(size_t)L - 1] = cur;
   }
   for (int l = L - 2; l >= 0; l--)
   {
      double       *cur = sol[(size_t)l], *alt = spare[(size_t)l];
      const double *fl  = l == 0 ? B : multi_work_[(size_t)l].f.data();
      spmm(levels[(size_t)l].P, K, MM_PLAIN, 1.0, sol[(size_t)l + 1], 1.0, cur, nullptr, nullptr, nullptr, cur, -1);
      sweeps(l, 1, prm.sweeps_up, false, fl, cur, alt);
      sol[(size_t)l] = cur;
   }
   if (sol[0] != X) multi_copy(level_A(0).nrows, K, sol[0], X);
}

double Amg::vcycle_multi_bytes(int K) const
{
   const int L     = num_levels();
   double    bytes = 0.0;
   for (int l = 0; l < L - 1; l++)
   {
      const DCsr &A = level_A(l);
      bytes += 24.0 * K * A.nrows * (prm.sweeps_down > 0 ? 1 : 0);                                              // scale: f, out (+ d)
      bytes += spmm_bytes(A, K, MM_JACOBI, false) * (std::max(prm.sweeps_down - 1, 0) + prm.sweeps_up);         // sweeps
      bytes += spmm_bytes(A, K, MM_RESID, false) + spmm_bytes(levels[(size_t)l].R, K, MM_PLAIN, false);         // residual, restriction
      bytes += spmm_bytes(levels[(size_t)l].P, K, MM_PLAIN, false) + 8.0 * K * A.nrows;                         // prolongation with add
   }
   bytes += coarse_dense ? 8.0 * coarse_n * (double)coarse_n + 16.0 * K * coarse_n : spmm_bytes(level_A(L - 1), K, MM_JACOBI, false);
   return bytes;
}

// ------------------------------------------------------- k PCG recurrences in lockstep

std::vector<KrylovResult> pcg_multi(const DCsr &A, Amg *amg, const KrylovParams &kp, int k, const double *B, double *X)
{
   const std::string why = multi_refusal(k);
   if (!why.empty()) throw Error(why);
   HDA_REQUIRE(A.nrows == A.ncols, "pcg_multi: a square operator on one rank is required");
   Context      &ctx = Context::get();
   MultiScratch &m   = MultiScratch::get();
   const int     n = A.nrows, K = multi_width(k);
   const size_t  vl = (size_t)std::max(n, 1) * K;
   std::vector<KrylovResult> res((size_t)k);
   DArray<double>            r(vl), p(vl), s(vl);
   auto precond = [&](const double *rr, double *zz) {
      for (KrylovResult &q : res) q.precond_calls++;
      if (amg) amg->apply_multi(rr, zz, K);
      else multi_copy(n, K, rr, zz);
   };
   auto read_blocks = [&](int first, int count) {
      multi_read_scalars_async(first, count);
      wait_event(ctx.ev);
   };
   // bi_prod_j = <b_j, b_j> (two_norm) or <C b_j, b_j>
   if (kp.two_norm) multi_dot(n, K, B, B, MS_TMP);
   else
   {
      precond(B, p.data());
      multi_dot(n, K, B, p.data(), MS_TMP);
   }
   multi_finalize(K, MS_TMP, 1, MV_BB);
   read_blocks(MV_BB, 1);
   double   bi[kMultiMax], eps[kMultiMax], i_prod[kMultiMax];
   int      active[kMultiMax];
   unsigned zero_rhs = 0;
   int      nactive  = 0;
   for (int j = 0; j < kMultiMax; j++)
   {
      bi[j]     = j < k ? m.host(MV_BB)[j] : 0.0;
      i_prod[j] = 0.0;
      active[j] = j < k && bi[j] != 0.0;
      nactive += active[j];
      if (j < k && bi[j] == 0.0)
      { // hypre: zero rhs => x = b = 0, no iteration
         zero_rhs |= 1u << j;
         res[(size_t)j].hist.push_back(0.0);
      }
      eps[j] = kp.rtol * kp.rtol;
      if (active[j] && kp.atol * kp.atol / bi[j] > eps[j]) eps[j] = kp.atol * kp.atol / bi[j];
   }
   multi_copy_columns(n, K, zero_rhs, B, X);
   if (nactive == 0)
   {
      ctx.sync();
      return res;
   }
   multi_set_active(active);
   // r = b - A x ; p = C r ; gamma = <r,p>
   spmm(A, K, MM_RESID, 1.0, X, 0.0, nullptr, B, nullptr, nullptr, r.data(), -1);
   precond(r.data(), p.data());
   multi_dot(n, K, r.data(), p.data(), MS_GAMMA);
   multi_dot(n, K, r.data(), r.data(), MS_RR);
   multi_finalize(K, MS_GAMMA, 2, MV_GAMMA0);
   read_blocks(MV_GAMMA0, 2);
   for (int j = 0; j < k; j++)
      if (active[j])
      {
         i_prod[j] = kp.two_norm ? m.host(MV_RR0)[j] : m.host(MV_GAMMA0)[j];
         res[(size_t)j].hist.push_back(std::sqrt(std::fabs(i_prod[j])));
      }
   int it = 0;
   while (it + 1 <= kp.max_iter && nactive > 0)
   {
      it++;
      const int go = (it & 1) ? MV_GAMMA0 : MV_GAMMA1, gn = (it & 1) ? MV_GAMMA1 : MV_GAMMA0, rn = gn + 1;
      spmm(A, K, MM_PLAIN, 1.0, p.data(), 0.0, nullptr, nullptr, nullptr, p.data(), s.data(), MS_SP);
      multi_cg_alpha(K, go);
      multi_cg_update(n, K, m.block(MV_ALPHA), p.data(), s.data(), X, r.data(), MS_RR);
      precond(r.data(), s.data());
      multi_dot(n, K, r.data(), s.data(), MS_GAMMA);
      multi_cg_beta(K, go, gn);
      multi_read_scalars_async(MV_GAMMA0, 5); // <r,z>, <r,r> of both parities and <s,p>: K doubles each
      multi_cg_dir(n, K, m.block(MV_BETA), s.data(), p.data());
      wait_event(ctx.ev);
      bool changed = false;
      for (int j = 0; j < k; j++)
      {
         if (!active[j]) continue;
         KrylovResult &q  = res[(size_t)j];
         const double  sp = m.host(MV_SP)[j];
         if (sp == 0.0 || !std::isfinite(sp))
         { // hypre: <s,p> == 0 is a breakdown, the update was not meaningful (and alpha_j was 0: x_j is untouched)
            q.iters   = it - 1;
            active[j] = 0;
            changed   = true;
            continue;
         }
         i_prod[j] = kp.two_norm ? m.host(rn)[j] : m.host(gn)[j];
         q.hist.push_back(std::sqrt(std::fabs(i_prod[j])));
         if (i_prod[j] / bi[j] < eps[j])
         {
            q.converged = true;
            q.iters     = it;
            active[j]   = 0;
            changed     = true;
         }
      }
      if (changed)
      {
         nactive = 0;
         for (int j = 0; j < k; j++) nactive += active[j];
         multi_set_active(active);
      }
   }
   for (int j = 0; j < k; j++)
   {
      if (active[j]) res[(size_t)j].iters = it;
      if (bi[j] != 0.0) res[(size_t)j].final_rel = std::sqrt(std::fabs(i_prod[j]) / bi[j]);
   }
   ctx.sync();
   return res;
}

} // namespace hda
