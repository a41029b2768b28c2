// hda_ilu.hip -- block-Jacobi ILU(0): hypre's "bj-iluk" with fill level 0 and no local
// reordering, the configuration the reference builds in hypredrv_ILUCreate
// (src/internal/ilu.c:63-115, defaults :15-28) and, as BoomerAMG's complex smoother, in
// src/internal/amg.c:899-921.  hypre is not part of the reference tree; the arithmetic is the
// textbook IKJ ILU(0) on the rank's diagonal block (ghost columns dropped), rows in natural
// order -- the definition the CPU checker of the test suite restates.  PARITY UNPINNED
// against hypre: no checked-in reference output uses ILU on data that is present.
//
// Device mapping.  Factorising row i needs the finished rows k < i it is coupled to, and the
// two substitutions have the same dependency DAG, so all three reuse the dependency levels
// of the Gauss-Seidel plan (hda_gs.hip): rows of one level are mutually non-adjacent, a
// level is one data-parallel launch, runs of small levels are fused into one workgroup with
// barriers.  The factorisation applies its updates to an entry in ascending pivot order
// whatever the schedule, so the factors are bit-identical to the sequential algorithm.
// tri_solve = 0 replaces the substitutions by Jacobi iterations on the triangular systems
// (ilu.c:21-23): plain streaming passes, the form that suits the GPU.
#include "hda_amg.h"

#include <algorithm>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

enum { OP_FACTOR = 0, OP_LOWER = 1, OP_UPPER = 2 };
constexpr int kLanes = 8; // lanes per row in the substitutions

// the row block of row i: [lo, hi) (part == nullptr: the whole diagonal block [0, n))
__device__ __forceinline__ void ilu_block_of(int i, int n, const int *__restrict__ part, int nb, int &lo, int &hi)
{
   lo = 0;
   hi = n;
   if (!part) return;
   int a = 0, b = nb; // part[a] <= i < part[b]
   while (b - a > 1)
   {
      const int m = (a + b) >> 1;
      if (part[m] <= i) a = m;
      else b = m;
   }
   lo = part[a];
   hi = part[b];
}

__global__ __launch_bounds__(256) void k_ilu_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const int *__restrict__ part,
                                                   int nb, int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int lo, hi, c = 0;
   ilu_block_of(i, n, part, nb, lo, hi);
   for (int k = rp[i]; k < rp[i + 1]; k++) c += (cj[k] >= lo && cj[k] < hi);
   cnt[i] = c;
}

// copy the diagonal block; flag bit 0: a row without diagonal entry, bit 1: a row that is not column-sorted
__global__ __launch_bounds__(256) void k_ilu_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                  const int *__restrict__ part, int nb, const int *__restrict__ orp, int *__restrict__ ocj,
                                                  double *__restrict__ ov, int *__restrict__ diag, int *flag)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int q = orp[i], d = -1, prev = -1, bad = 0, lo, hi;
   ilu_block_of(i, n, part, nb, lo, hi);
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int j = cj[k];
      if (j < lo || j >= hi) continue;
      if (j <= prev) bad = 2;
      prev = j;
      if (j == i) d = q;
      ocj[q] = j;
      ov[q]  = v[k];
      q++;
   }
   diag[i] = d;
   if (d < 0) bad |= 1;
   if (bad) atomicOr(flag, bad);
}

__global__ __launch_bounds__(256) void k_ilu_diag(int n, const int *__restrict__ rp, const int *__restrict__ cj, int *__restrict__ diag)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int d = -1;
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (cj[k] == i) d = k;
   diag[i] = d;
}

// one row of the IKJ factorisation (Saad, Alg. 10.4): for every k < i of the row in ascending order,
// l_ik = a_ik / u_kk, then a_ij -= l_ik u_kj for the j > k that row i holds
__device__ __forceinline__ void ilu_factor_row(int i, const int *__restrict__ rp, const int *__restrict__ cj, double *v,
                                               const int *__restrict__ dg, int *flag)
{
   const int e = rp[i + 1], di = dg[i];
   for (int kk = rp[i]; kk < di; kk++)
   {
      const int    k   = cj[kk];
      const double lik = v[kk] / v[dg[k]];
      v[kk]            = lik;
      int pi = kk + 1;
      for (int jj = dg[k] + 1; jj < rp[k + 1]; jj++)
      {
         const int j = cj[jj];
         while (pi < e && cj[pi] < j) pi++;
         if (pi == e) break;
         if (cj[pi] == j) v[pi] -= lik * v[jj];
      }
   }
   if (v[di] == 0.0) atomicOr(flag, 4);
}

// rows [first, first + count) of the level permutation
template <int OP>
__device__ __forceinline__ void ilu_rows(int first, int count, int tid, int nthreads, const int *__restrict__ perm,
                                         const int *__restrict__ rp, const int *__restrict__ cj, double *v,
                                         const int *__restrict__ dg, double *x, int *flag)
{
   if (OP == OP_FACTOR)
   {
      for (int q = tid; q < count; q += nthreads) ilu_factor_row(perm[first + q], rp, cj, v, dg, flag);
      return;
   }
   const int lane = tid & (kLanes - 1);
   for (int q = tid / kLanes; q < count; q += nthreads / kLanes)
   {
      const int i  = perm[first + q];
      const int lo = (OP == OP_LOWER) ? rp[i] : dg[i] + 1, hi = (OP == OP_LOWER) ? dg[i] : rp[i + 1];
      double    s  = 0.0;
      for (int k = lo + lane; k < hi; k += kLanes) s += v[k] * x[cj[k]];
#pragma unroll
      for (int o = kLanes / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) x[i] = (OP == OP_LOWER) ? (x[i] - s) : (x[i] - s) / v[dg[i]];
   }
}

template <int OP>
__global__ __launch_bounds__(256) void k_ilu_level(int first, int count, const int *__restrict__ perm, const int *__restrict__ rp,
                                                   const int *__restrict__ cj, double *v, const int *__restrict__ dg, double *x, int *flag)
{
   ilu_rows<OP>(first, count, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, perm, rp, cj, v, dg, x, flag);
}

// levels [l0, l1) by one workgroup, ascending (factor, lower) or descending (upper), a barrier between levels
template <int OP>
__global__ __launch_bounds__(1024) void k_ilu_fused(int l0, int l1, const int *__restrict__ lvl_ptr, const int *__restrict__ perm,
                                                    const int *__restrict__ rp, const int *__restrict__ cj, double *v,
                                                    const int *__restrict__ dg, double *x, int *flag)
{
   for (int s = 0; s < l1 - l0; s++)
   {
      const int L = (OP == OP_UPPER) ? (l1 - 1 - s) : (l0 + s);
      ilu_rows<OP>(lvl_ptr[L], lvl_ptr[L + 1] - lvl_ptr[L], threadIdx.x, blockDim.x, perm, rp, cj, v, dg, x, flag);
      __threadfence_block();
      __syncthreads();
   }
}

template <int OP>
void run_levels(const DCsr &LU, const GsPlan &p, const int *dg, double *x, int *flag)
{
   const int ns  = (int)p.segments.size();
   double   *v   = const_cast<double *>(LU.val.data());
   const int per = (OP == OP_FACTOR) ? 1 : kLanes;
   for (int si = 0; si < ns; si++)
   {
      const auto &sg    = p.segments[(size_t)(OP == OP_UPPER ? ns - 1 - si : si)];
      const int   first = p.lvl_ptr[(size_t)sg.first], count = p.lvl_ptr[(size_t)sg.first + 1] - first;
      if (sg.second - sg.first == 1 && count > 512)
         k_ilu_level<OP><<<std::min(ceil_div((long long)count * per, 256), 2048), 256, 0, STREAM>>>(
            first, count, p.perm.data(), LU.rowptr.data(), LU.col.data(), v, dg, x, flag);
      else
         k_ilu_fused<OP><<<1, 1024, 0, STREAM>>>(sg.first, sg.second, p.d_lvl_ptr.data(), p.perm.data(), LU.rowptr.data(), LU.col.data(),
                                                 v, dg, x, flag);
   }
}

__global__ __launch_bounds__(256) void k_ilu_block_divisors(int n, const double *__restrict__ v, const int *__restrict__ dg, double *__restrict__ ones,
                                                            double *__restrict__ udinv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   ones[i]  = 1.0;
   udinv[i] = 1.0 / v[dg[i]];
}

// split the factors for the Jacobi-iterative solves: Ls = strict lower part, Us = diagonal + strict upper part
__global__ __launch_bounds__(256) void k_ilu_split_count(int n, const int *__restrict__ rp, const int *__restrict__ dg, int *__restrict__ nl,
                                                         int *__restrict__ nu)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   nl[i] = dg[i] - rp[i];
   nu[i] = rp[i + 1] - dg[i];
}
__global__ __launch_bounds__(256) void k_ilu_split_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                        const int *__restrict__ dg, const int *__restrict__ lrp, int *__restrict__ lcj,
                                                        double *__restrict__ lv, const int *__restrict__ urp, int *__restrict__ ucj,
                                                        double *__restrict__ uv, double *__restrict__ dinv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int q = lrp[i];
   for (int k = rp[i]; k < dg[i]; k++, q++) { lcj[q] = cj[k]; lv[q] = v[k]; }
   q = urp[i];
   for (int k = dg[i]; k < rp[i + 1]; k++, q++) { ucj[q] = cj[k]; uv[q] = v[k]; }
   dinv[i] = 1.0 / v[dg[i]];
}

} // namespace

void Ilu::setup(const DCsr &A, const IluParams &p)
{
   prm         = p;
   prm.lower_it = std::max(p.lower_it, 1);
   prm.upper_it = std::max(p.upper_it, 1);
   const int n = A.nrows;
   LU          = DCsr();
   LU.nrows = LU.ncols = n;
   LU.rowptr.alloc((size_t)n + 1);
   diag.alloc((size_t)std::max(n, 1));
   DArray<int> cnt((size_t)n + 1), flag(1);
   cnt.zero();
   flag.zero();
   // row blocks: the caller's starts, hypre's even split into V, or the setup's own choice (blocks = 0)
   bpart.clear();
   bplan = GsPlan();
   {
      int V = prm.blocks;
      if (V == 0) V = amg_auto_blocks(A);
      V = std::min(std::max(V, 1), std::max(n, 1));
      if (!prm.block_part.empty())
      {
         HDA_REQUIRE((int)prm.block_part.size() == V + 1 && prm.block_part.front() == 0 && prm.block_part.back() == n,
                     "ILU: block_part must hold blocks + 1 ascending row starts from 0 to the number of rows");
         bpart.assign(prm.block_part.begin(), prm.block_part.end());
      }
      else if (V > 1)
      {
         bpart.resize((size_t)V + 1);
         for (int q = 0; q <= V; q++) bpart[(size_t)q] = (int)(((__int128)q * n) / V);
      }
      if (bpart.size() <= 2) bpart.clear();
   }
   const int   nb = bpart.empty() ? 0 : (int)bpart.size() - 1;
   DArray<int> dpart;
   if (nb) dpart.upload(bpart.data(), bpart.size());
   const int *pp = nb ? dpart.data() : nullptr;
   if (n) k_ilu_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), pp, nb, cnt.data());
   require_int32_total(n, cnt.data(), "ILU factor");
   exclusive_scan(n, cnt.data(), LU.rowptr.data(), nullptr);
   HDA_HIP(hipMemcpyAsync(&LU.nnz, LU.rowptr.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   LU.col.alloc((size_t)std::max(LU.nnz, 1));
   LU.val.alloc((size_t)std::max(LU.nnz, 1));
   if (n)
      k_ilu_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), pp, nb, LU.rowptr.data(), LU.col.data(),
                                                      LU.val.data(), diag.data(), flag.data());
   int f = 0;
   flag.download(&f, 1);
   HDA_REQUIRE(!(f & 1), "ILU(0): a row of the diagonal block has no diagonal entry");
   if (f & 2)
   { // e.g. a level whose rows were left unsorted by the solve-phase renumbering
      sort_rows(LU);
      k_ilu_diag<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, LU.rowptr.data(), LU.col.data(), diag.data());
   }
   HDA_REQUIRE(!(factor_and_plan() & 4), "ILU(0): zero pivot");
}

// the internal entry behind a caller that brings its own pattern (the Schwarz subdomain solves, hda_schwarz.hip): P holds the
// pattern of the factors, column-sorted, every row with its diagonal entry, the operator's values scattered in and zeros at the
// fill positions; part = the row starts of its diagonal blocks (empty or one block: none).  Returns the factorisation's flags
// (bit 2: a zero pivot) instead of throwing, so that the caller can name what it factorised.
int Ilu::setup_pattern(DCsr &&P, const IluParams &p, const std::vector<int> &part)
{
   prm          = p;
   prm.lower_it = std::max(p.lower_it, 1);
   prm.upper_it = std::max(p.upper_it, 1);
   LU           = std::move(P);
   const int n  = LU.nrows;
   diag.alloc((size_t)std::max(n, 1));
   bpart = part;
   if (bpart.size() <= 2) bpart.clear();
   bplan = GsPlan();
   if (n) k_ilu_diag<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, LU.rowptr.data(), LU.col.data(), diag.data());
   return factor_and_plan();
}

// numeric factorisation of LU on its dependency levels, then what the substitutions need; returns the flags (bit 2: zero pivot)
int Ilu::factor_and_plan()
{
   const int   n  = LU.nrows;
   const int   nb = bpart.empty() ? 0 : (int)bpart.size() - 1;
   int         f  = 0;
   DArray<int> flag(1);
   build_gs_plan(LU, plan);
   flag.zero();
   run_levels<OP_FACTOR>(LU, plan, diag.data(), nullptr, flag.data());
   flag.download(&f, 1);
   if (f & 4) return f;
   work.alloc((size_t)std::max(n, 1) * 2);
   Ls = DCsr();
   Us = DCsr();
   if (prm.tri_solve && nb && n)
   { // the substitutions on the block kernels: the plan copies the FINISHED factors into sweep order
      build_gs_plan_blocks(LU, bpart, bplan);
      ones.alloc((size_t)n);
      udinv.alloc((size_t)n);
      k_ilu_block_divisors<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, LU.val.data(), diag.data(), ones.data(), udinv.data());
   }
   if (!prm.tri_solve && n)
   { // the iterations are plain products with the two triangles: keep each in its own CSR so that a pass
     // streams only its half, through the same kernels (and launch plans) as every other operator
      DArray<int> nl((size_t)n + 1), nu((size_t)n + 1);
      nl.zero();
      nu.zero();
      k_ilu_split_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, LU.rowptr.data(), diag.data(), nl.data(), nu.data());
      Ls.nrows = Ls.ncols = Us.nrows = Us.ncols = n;
      Ls.rowptr.alloc((size_t)n + 1);
      Us.rowptr.alloc((size_t)n + 1);
      exclusive_scan(n, nl.data(), Ls.rowptr.data(), nullptr);
      exclusive_scan(n, nu.data(), Us.rowptr.data(), nullptr);
      HDA_HIP(hipMemcpyAsync(&Ls.nnz, Ls.rowptr.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
      HDA_HIP(hipMemcpyAsync(&Us.nnz, Us.rowptr.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
      Context::get().sync();
      Ls.col.alloc((size_t)std::max(Ls.nnz, 1));
      Ls.val.alloc((size_t)std::max(Ls.nnz, 1));
      Us.col.alloc((size_t)std::max(Us.nnz, 1));
      Us.val.alloc((size_t)std::max(Us.nnz, 1));
      dinv.alloc((size_t)n);
      k_ilu_split_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, LU.rowptr.data(), LU.col.data(), LU.val.data(), diag.data(), Ls.rowptr.data(),
                                                            Ls.col.data(), Ls.val.data(), Us.rowptr.data(), Us.col.data(), Us.val.data(),
                                                            dinv.data());
      spmv_prepare(Ls);
      spmv_prepare(Us);
   }
   return f;
}

// z = U^{-1} L^{-1} r   (r and z may not alias)
void Ilu::apply(const double *r, double *z)
{
   const int n = LU.nrows;
   if (n == 0) return;
   if (prm.tri_solve && bplan.built)
   { // row blocks: y = L^-1 r is a forward block sweep over LU from the zero guess with unit divisors (y_i = r_i - sum_{j<i} l_ij y_j:
     // the diagonal and the upper entries multiply zeros), z = U^-1 y a backward one with 1 / u_ii (the lower entries do)
      double *y = work.data();
      gs_sweep_blocks(LU, bplan, ones.data(), r, nullptr, y, true, true);
      gs_sweep_blocks(LU, bplan, udinv.data(), y, nullptr, z, false, true);
      return;
   }
   if (prm.tri_solve)
   {
      copy(n, r, z);
      run_levels<OP_LOWER>(LU, plan, diag.data(), z, nullptr);
      run_levels<OP_UPPER>(LU, plan, diag.data(), z, nullptr);
      return;
   }
   // Jacobi iterations from a zero guess: the first one is y = r (resp. z = D^{-1} y); then
   // y <- r - L~ y is a residual with the strict lower triangle, and z <- D^{-1}(y - U~ z) is a Jacobi
   // sweep z + D^{-1}(y - (D + U~) z) with the upper triangle that includes the diagonal
   double       *ya = work.data(), *yb = work.data() + n;
   const double *y = r;
   for (int it = 1; it < prm.lower_it; it++)
   {
      double *out = (it & 1) ? ya : yb;
      residual(Ls, y, r, out);
      y = out;
   }
   // y now lives in r, ya or yb; the upper iterations ping-pong between z and the free half of work
   double *spare = (y == ya) ? yb : ya;
   mul(n, dinv.data(), y, (prm.upper_it & 1) ? z : spare);
   const double *zin = (prm.upper_it & 1) ? z : spare;
   for (int it = 1; it < prm.upper_it; it++)
   {
      double *out = (zin == z) ? spare : z;
      jacobi(Us, dinv.data(), y, zin, out, -1);
      zin = out;
   }
   // upper_it - 1 swaps starting from the buffer chosen above end in z
}

// algorithmic HBM bytes of one apply (factors once per pass, vectors in and out)
double Ilu::apply_bytes() const
{
   const double n = LU.nrows;
   if (prm.tri_solve) return 2.0 * (12.0 * LU.nnz / 2.0 + 8.0 * n + 24.0 * n) + 16.0 * n; // two substitutions over half the pattern each + the copy
   const double lower = 12.0 * Ls.nnz + 4.0 * (n + 1) + 24.0 * n, upper = 12.0 * Us.nnz + 4.0 * (n + 1) + 32.0 * n;
   return (prm.lower_it - 1) * lower + 24.0 * n + (prm.upper_it - 1) * upper;
}

} // namespace hda
