// hda_fsai.hip -- static factorised sparse approximate inverse ("preconditioner: fsai", algo_type bj-sfsai).
// hypre is not part of the reference tree, so the algorithm is this project's own definition in the spirit of hypre's static power
// pattern (tests/fsai_reference.py is the same definition on the host).  PARITY UNPINNED against hypre.
//
//   pattern   S = D^-1/2 |A| D^-1/2 with the off-diagonal entries below `threshold` dropped; K_1 = S, K_(l+1) = K_l S (numeric product
//             of non-negative matrices, the same drop after every product); K = K_num_levels
//   rows      P_i = { j < i : K_ij kept, j inside i's row block } + { i }; more than max_nnz_row entries: i and the max_nnz_row - 1
//             candidates of largest K_ij, ties to the larger column; ascending, diagonal last
//   values    M = A[P_i, P_i] from the stored entries (lower triangle; absent = 0), M = L L^T without pivoting, g_i = L^-T e_last --
//             that is y / sqrt(y_last) of M y = e_last.  A pivot <= 0: the row is the single entry 1 / sqrt(a_ii), and is counted
//   omega     1 / lambda after eig_max_iters power steps on G^T G A from a fixed start vector; 0 steps: 1
//   apply     z = omega G^T (G r): two products on the SpMV family with an explicit G^T -- no atomic scatter, bitwise reproducible
//
// The local systems (k_fsai_local) are the hot kernel of the setup.  A row with s = |P_i| entries gets LPR = 4, 8, 16, 32 or 64 lanes
// (the smallest that holds s); a block is ONE wavefront that works on 64 / LPR rows of one class at a time.  Lane t of a row's group
// owns row t of M: it gathers it by merging the column-sorted row P_i[t] of A with the sorted P_i, then the right-looking Cholesky
// and the back substitution run in lockstep over the columns.  M lives in LDS as the packed lower triangle, LPR (LPR + 1) / 2 doubles
// per row of G: 16.5 KiB per wavefront in the 64-lane class (9 wavefronts per CU of 160 KiB), 4.5 KiB in the 16-lane class.  Results
// leave through plain stores, one lane per entry of G; the classes' row lists come from scans.  No atomics anywhere.
#include "hda_amg.h"

#include <algorithm>
#include <cmath>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

constexpr int kFsaiMaxRow = 64; // max_nnz_row: one wavefront's worth

__device__ __forceinline__ int fs_block_start(int i, const int *__restrict__ part, int V)
{
   int a = 0, b = V; // part[a] <= i < part[b]
   while (b - a > 1)
   {
      const int m = (a + b) >> 1;
      if (part[m] <= i) a = m;
      else b = m;
   }
   return part[a];
}

// S = D^-1/2 |A| D^-1/2 on the pattern of A (values only; ghost columns get 0 and are dropped by the filter that follows)
__global__ __launch_bounds__(256) void k_fsai_scale(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ av,
                                                    const double *__restrict__ d, double *__restrict__ sv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   const double di = d[i];
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int j = cj[k];
      sv[k]       = (j < n) ? fabs(av[k]) / sqrt(di * d[j]) : -1.0;
   }
}
// the diagonal and the off-diagonal entries >= tau of a square matrix: count pass, fill pass
template <bool FILL>
__global__ __launch_bounds__(256) void k_fsai_drop(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v, double tau,
                                                   int *__restrict__ cnt, const int *__restrict__ orp, int *__restrict__ ocj, double *__restrict__ ov)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int o = FILL ? orp[i] : 0;
   for (int k = rp[i]; k < rp[i + 1]; k++)
   {
      const int j = cj[k];
      if (j >= n || (j != i && !(v[k] >= tau))) continue;
      if (FILL)
      {
         ocj[o] = j;
         ov[o]  = v[k];
      }
      o++;
   }
   if (!FILL) cnt[i] = o;
}
// row selection: one wavefront per row of K.  keep[k] = 1 for the chosen off-diagonal candidates, cnt[i] = |P_i|
__global__ __launch_bounds__(64) void k_fsai_select(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v, int m,
                                                    const int *__restrict__ part, int V, unsigned char *__restrict__ keep, int *__restrict__ cnt)
{
   const int lane = threadIdx.x;
   for (int i = blockIdx.x; i < n; i += gridDim.x)
   {
      const int b = rp[i], e = rp[i + 1], lo = fs_block_start(i, part, V);
      int       c = 0;
      for (int k0 = b; k0 < e; k0 += 64)
      {
         const int  k    = k0 + lane;
         const bool cand = k < e && cj[k] < i && cj[k] >= lo;
         c += __popcll(__ballot(cand));
      }
      if (c <= m - 1)
      {
         for (int k = b + lane; k < e; k += 64) keep[k] = (cj[k] < i && cj[k] >= lo) ? 1 : 0;
      }
      else
      { // rank of a candidate = the candidates ahead of it: larger value, or the same value and a larger column
         for (int k = b + lane; k < e; k += 64)
         {
            const int j = cj[k];
            int       take = 0;
            if (j < i && j >= lo)
            {
               const double x = v[k];
               int          rank = 0;
               for (int q = b; q < e; q++)
               {
                  const int    jq = cj[q];
                  const double xq = v[q];
                  if (jq < i && jq >= lo && (xq > x || (xq == x && jq > j))) rank++;
               }
               take = rank < m - 1;
            }
            keep[k] = (unsigned char)take;
         }
      }
      if (lane == 0) cnt[i] = min(c, m - 1) + 1;
   }
}
__global__ __launch_bounds__(256) void k_fsai_pattern(int n, const int *__restrict__ rp, const int *__restrict__ cj, const unsigned char *__restrict__ keep,
                                                      const int *__restrict__ grp, int *__restrict__ gcj)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int o = grp[i];
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (keep[k]) gcj[o++] = cj[k];
   gcj[o] = i;
}
// rows of one lane class: flag, (scan), list
__device__ __forceinline__ int fs_class(int s) { return s <= 4 ? 0 : s <= 8 ? 1 : s <= 16 ? 2 : s <= 32 ? 3 : 4; }
__global__ __launch_bounds__(256) void k_fsai_class_flag(int n, const int *__restrict__ grp, int cls, int *__restrict__ flag)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) flag[i] = fs_class(grp[i + 1] - grp[i]) == cls;
}
__global__ __launch_bounds__(256) void k_fsai_list(int n, const int *__restrict__ pos, int *__restrict__ list)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && pos[i + 1] > pos[i]) list[pos[i]] = i;
}

// ---------------------------------------------------------------- the local systems
template <int LPR>
__global__ __launch_bounds__(64) void k_fsai_local(int count, const int *__restrict__ rows, const int *__restrict__ arp, const int *__restrict__ acj,
                                                   const double *__restrict__ av, const int *__restrict__ grp, const int *__restrict__ gcj,
                                                   double *__restrict__ gv, int *__restrict__ fell)
{
   constexpr int G = 64 / LPR, TRI = LPR * (LPR + 1) / 2;
   __shared__ double Ms[G * TRI];
   __shared__ int    Ps[G * LPR];
   const int lane = threadIdx.x, g = lane / LPR, t = lane % LPR;
   const int q    = blockIdx.x * G + g;
   int       i = -1, o = 0, s = 0;
   if (q < count)
   {
      i = rows[q];
      o = grp[i];
      s = min(grp[i + 1] - o, LPR);
   }
   double   *M = Ms + g * TRI;
   int      *P = Ps + g * LPR;
   double   *Mt = M + t * (t + 1) / 2; // row t of the packed lower triangle
   if (t < s) P[t] = gcj[o + t];
   __syncthreads();
   // gather row t of M = A[P, P]: the sorted row P[t] of A against P[0..t]
   double att = 0.0;
   if (t < s)
   {
      for (int c = 0; c <= t; c++) Mt[c] = 0.0;
      const int r = P[t];
      int       c = 0;
      for (int k = arp[r]; k < arp[r + 1] && c <= t; k++)
      {
         const int j = acj[k];
         while (c <= t && P[c] < j) c++;
         if (c <= t && P[c] == j) Mt[c++] = av[k];
      }
      att = Mt[t];
   }
   int smax = s;
   for (int off = 32; off; off >>= 1) smax = max(smax, __shfl_xor(smax, off));
   __syncthreads();
   // right-looking Cholesky, column after column; the pivot is read by every lane of the group, so `failed` is uniform in it
   bool failed = false;
   for (int k = 0; k < smax; k++)
   {
      const bool   in  = k < s && !failed;
      const double piv = in ? M[k * (k + 1) / 2 + k] : 1.0;
      if (!(piv > 0.0)) failed = true;
      const bool   work = in && !failed && t > k && t < s;
      const double l    = sqrt(piv);
      if (work) Mt[k] /= l;
      __syncthreads();
      if (in && !failed && t == k) Mt[k] = l;
      if (work)
      {
         const double ltk = Mt[k];
         for (int c = k + 1; c <= t; c++) Mt[c] -= ltk * M[c * (c + 1) / 2 + k];
      }
      __syncthreads();
   }
   // L^T g = e_last, column-oriented: lane t collects sum_{r > t} L[r][t] g_r
   double acc = 0.0, gt = 0.0;
   for (int r = smax - 1; r >= 0; r--)
   {
      double gr = 0.0;
      if (t == r && r < s && !failed)
      {
         gr = ((r == s - 1 ? 1.0 : 0.0) - acc) / Mt[t];
         gt = gr;
      }
      gr = __shfl(gr, r, LPR);
      if (!failed && t < r && r < s) acc += M[r * (r + 1) / 2 + t] * gr;
   }
   if (t < s) gv[o + t] = failed ? (t == s - 1 ? 1.0 / sqrt(att) : 0.0) : gt;
   if (t == 0 && s > 0) fell[i] = failed ? 1 : 0;
}

// a factor with fallback rows: those rows keep their diagonal entry alone
template <bool FILL>
__global__ __launch_bounds__(256) void k_fsai_compact(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                      const int *__restrict__ fell, int *__restrict__ cnt, const int *__restrict__ orp,
                                                      int *__restrict__ ocj, double *__restrict__ ov)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   const int b = fell[i] ? rp[i + 1] - 1 : rp[i], e = rp[i + 1];
   if (!FILL)
   {
      cnt[i] = e - b;
      return;
   }
   int o = orp[i];
   for (int k = b; k < e; k++, o++)
   {
      ocj[o] = cj[k];
      ov[o]  = v[k];
   }
}
// z_i = ((i * 2654435761) mod 2^32) / 2^32 - 0.5, in integers: the host reference starts from the same doubles
__global__ __launch_bounds__(256) void k_fsai_start(int n, double *__restrict__ z)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) z[i] = (double)(unsigned int)((unsigned long long)i * 2654435761ull) / 4294967296.0 - 0.5;
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
// B = the diagonal and the off-diagonal entries >= tau of the n x n pattern (rp, cj) with the values v
void drop_small(int n, const int *rp, const int *cj, const double *v, double tau, DCsr &B)
{
   B.nrows = B.ncols = n;
   B.rowptr.alloc((size_t)n + 1);
   DArray<int> cnt((size_t)n + 1);
   cnt.zero();
   k_fsai_drop<false><<<ceil_div(n, 256), 256, 0, STREAM>>>(n, rp, cj, v, tau, cnt.data(), nullptr, nullptr, nullptr);
   require_int32_total(n, cnt.data(), "FSAI pattern");
   exclusive_scan(n, cnt.data(), B.rowptr.data(), nullptr);
   B.nnz = last_of(B.rowptr, (size_t)n);
   B.col.alloc((size_t)std::max(B.nnz, 1));
   B.val.alloc((size_t)std::max(B.nnz, 1));
   k_fsai_drop<true><<<ceil_div(n, 256), 256, 0, STREAM>>>(n, rp, cj, v, tau, nullptr, B.rowptr.data(), B.col.data(), B.val.data());
}
template <int LPR>
void launch_local(int count, const int *rows, const DCsr &A, DCsr &G, int *fell)
{
   constexpr int per = 64 / LPR;
   k_fsai_local<LPR><<<ceil_div(count, per), 64, 0, STREAM>>>(count, rows, A.rowptr.data(), A.col.data(), A.val.data(), G.rowptr.data(), G.col.data(),
                                                             G.val.data(), fell);
}

} // namespace

std::string fsai_params_refusal(const FsaiParams &p)
{
   if (p.num_levels < 1) return "FSAI: num_levels must be >= 1";
   if (!(p.threshold >= 0.0)) return "FSAI: threshold must be >= 0";
   if (p.max_nnz_row < 1) return "FSAI: max_nnz_row must be >= 1";
   if (p.max_nnz_row > kFsaiMaxRow)
      return "FSAI: max_nnz_row " + std::to_string(p.max_nnz_row) + " is not implemented on MI355X (at most 64, one wavefront's worth of a row)";
   if (p.eig_max_iters < 0) return "FSAI: eig_max_iters must be >= 0";
   if (p.max_iter < 1) return "FSAI: max_iter must be >= 1";
   return "";
}

void Fsai::setup(const DCsr &A, const FsaiParams &p, const std::vector<int> *part)
{
   prm = p;
   n   = A.nrows;
   {
      const std::string why = fsai_params_refusal(p);
      if (!why.empty()) throw Error(why);
   }
   // row blocks: the caller's starts, hypre's even split into V, or the setup's own choice (blocks = 0) -- as Ilu::setup
   std::vector<int> bpart;
   if (part && part->size() >= 2) bpart = *part;
   else
   {
      int nb = prm.blocks;
      if (nb == 0) nb = amg_auto_blocks(A);
      nb = std::min(std::max(nb, 1), std::max(n, 1));
      if (!prm.block_part.empty())
      {
         HDA_REQUIRE((int)prm.block_part.size() == nb + 1 && prm.block_part.front() == 0 && prm.block_part.back() == n,
                     "FSAI: block_part must hold blocks + 1 ascending row starts from 0 to the number of rows");
         for (size_t q = 1; q < prm.block_part.size(); q++) HDA_REQUIRE(prm.block_part[q] >= prm.block_part[q - 1], "FSAI: block_part must ascend");
         bpart.assign(prm.block_part.begin(), prm.block_part.end());
      }
      else
      {
         bpart.resize((size_t)nb + 1);
         for (int q = 0; q <= nb; q++) bpart[(size_t)q] = (int)(((__int128)q * n) / nb);
      }
   }
   HDA_REQUIRE(bpart.front() == 0 && bpart.back() == n, "FSAI: the row blocks must cover the rows of the operator");
   nblocks = (int)bpart.size() - 1;
   DArray<int> dpart;
   dpart.upload(bpart.data(), bpart.size());
   fallback_rows = 0;
   omega         = 1.0;
   G             = DCsr();
   GT            = DCsr();
   G.nrows = G.ncols = GT.nrows = GT.ncols = n;
   G.rowptr.alloc((size_t)n + 1);
   if (n == 0)
   {
      G.rowptr.zero();
      return;
   }
   double t0 = now_ms();
   // ---- the diagonal must be positive: the scaling and the fallback divide by its root
   DArray<double> d((size_t)n);
   extract_diag(A, d.data());
   {
      const std::vector<double> hd = d.to_host();
      for (int i = 0; i < n; i++)
         if (!(hd[(size_t)i] > 0.0))
         {
            char msg[200];
            snprintf(msg, sizeof msg, "FSAI: row %d has no positive stored diagonal entry (%g); the static pattern is defined for operators with a positive diagonal", i,
                     hd[(size_t)i]);
            throw Error(msg);
         }
   }
   // ---- pattern: S, K = S^num_levels with the drop after every product
   DCsr S, K;
   {
      DArray<double> sv((size_t)std::max(A.nnz, 1));
      k_fsai_scale<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A.rowptr.data(), A.col.data(), A.val.data(), d.data(), sv.data());
      drop_small(n, A.rowptr.data(), A.col.data(), sv.data(), prm.threshold, S);
   }
   for (int l = 1; l < prm.num_levels; l++)
   {
      DCsr X;
      spgemm(l == 1 ? S : K, S, X);
      DCsr Y;
      drop_small(n, X.rowptr.data(), X.col.data(), X.val.data(), prm.threshold, Y);
      K = std::move(Y);
   }
   const DCsr &Kp = prm.num_levels == 1 ? S : K;
   // ---- rows
   {
      DArray<unsigned char> keep((size_t)std::max(Kp.nnz, 1));
      DArray<int>           cnt((size_t)n + 1);
      cnt.zero();
      k_fsai_select<<<std::min(n, 65536), 64, 0, STREAM>>>(n, Kp.rowptr.data(), Kp.col.data(), Kp.val.data(), prm.max_nnz_row, dpart.data(), nblocks,
                                                          keep.data(), cnt.data());
      require_int32_total(n, cnt.data(), "FSAI factor");
      exclusive_scan(n, cnt.data(), G.rowptr.data(), nullptr);
      G.nnz = last_of(G.rowptr, (size_t)n);
      G.col.alloc((size_t)G.nnz);
      G.val.alloc((size_t)G.nnz);
      k_fsai_pattern<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, Kp.rowptr.data(), Kp.col.data(), keep.data(), G.rowptr.data(), G.col.data());
   }
   S = DCsr();
   K = DCsr();
   double t1 = now_ms();
   setup_ms[0] = t1 - t0;
   // ---- local systems, lane class after lane class
   {
      DArray<int> fell((size_t)n + 1), flag((size_t)n + 1), pos((size_t)n + 1), list((size_t)n);
      fell.zero();
      for (int cls = 0; cls < 5; cls++)
      {
         flag.zero();
         k_fsai_class_flag<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, G.rowptr.data(), cls, flag.data());
         exclusive_scan(n, flag.data(), pos.data(), nullptr);
         const int count = last_of(pos, (size_t)n);
         class_rows[cls] = count;
         if (count == 0) continue;
         k_fsai_list<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, pos.data(), list.data());
         if (cls == 0) launch_local<4>(count, list.data(), A, G, fell.data());
         else if (cls == 1) launch_local<8>(count, list.data(), A, G, fell.data());
         else if (cls == 2) launch_local<16>(count, list.data(), A, G, fell.data());
         else if (cls == 3) launch_local<32>(count, list.data(), A, G, fell.data());
         else launch_local<64>(count, list.data(), A, G, fell.data());
      }
      exclusive_scan(n, fell.data(), pos.data(), nullptr);
      fallback_rows = last_of(pos, (size_t)n);
      if (fallback_rows > 0)
      {
         DCsr C;
         C.nrows = C.ncols = n;
         C.rowptr.alloc((size_t)n + 1);
         flag.zero();
         k_fsai_compact<false><<<ceil_div(n, 256), 256, 0, STREAM>>>(n, G.rowptr.data(), G.col.data(), G.val.data(), fell.data(), flag.data(), nullptr,
                                                                    nullptr, nullptr);
         exclusive_scan(n, flag.data(), C.rowptr.data(), nullptr);
         C.nnz = last_of(C.rowptr, (size_t)n);
         C.col.alloc((size_t)C.nnz);
         C.val.alloc((size_t)C.nnz);
         k_fsai_compact<true><<<ceil_div(n, 256), 256, 0, STREAM>>>(n, G.rowptr.data(), G.col.data(), G.val.data(), fell.data(), nullptr, C.rowptr.data(),
                                                                   C.col.data(), C.val.data());
         G = std::move(C);
      }
   }
   double t2 = now_ms();
   setup_ms[1] = t2 - t1;
   // ---- G^T and the launch plans of both products
   transpose(G, GT);
   spmv_prepare(G);
   spmv_prepare(GT);
   work.alloc((size_t)n);
   double t3 = now_ms();
   setup_ms[2] = t3 - t2;
   // ---- omega = 1 / lambda after eig_max_iters power steps on G^T G A
   if (prm.eig_max_iters > 0)
   {
      DArray<double> z((size_t)std::max(A.ncols, n)), w((size_t)std::max(A.ncols, n)), az((size_t)n);
      z.zero();
      w.zero();
      k_fsai_start<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, z.data());
      double lambda = 0.0;
      for (int it = 0; it < prm.eig_max_iters; it++)
      {
         dot(n, z.data(), z.data(), 0);
         finalize(0, S_TMP);
         scale_inv_sqrt_dev(n, S_TMP, z.data());
         spmv(A, 1.0, z.data(), 0.0, nullptr, az.data());
         spmv(G, 1.0, az.data(), 0.0, nullptr, work.data());
         spmv(GT, 1.0, work.data(), 0.0, nullptr, w.data());
         if (it == prm.eig_max_iters - 1)
         {
            dot(n, w.data(), z.data(), 0);
            finalize(0, S_TMP);
            lambda = read_scalar(S_TMP);
         }
         std::swap(z, w);
      }
      if (!(lambda > 0.0))
      {
         char msg[200];
         snprintf(msg, sizeof msg, "FSAI: the eigenvalue estimate of G^T G A after eig_max_iters = %d steps is %g, not positive: no scaling omega", prm.eig_max_iters,
                  lambda);
         throw Error(msg);
      }
      omega = 1.0 / lambda;
   }
   setup_ms[3] = now_ms() - t3;
}

// z = omega G^T (G r); r and z must not alias the work vector, and may not alias each other
void Fsai::apply(const double *r, double *z)
{
   if (n == 0) return;
   spmv(G, 1.0, r, 0.0, nullptr, work.data());
   spmv(GT, omega, work.data(), 0.0, nullptr, z);
}

double Fsai::apply_bytes() const
{ // both products' (col, val) and row pointers, r read, the intermediate written and read, z written
   return 2.0 * (12.0 * G.nnz + 4.0 * (n + 1.0)) + 4.0 * 8.0 * n;
}

} // namespace hda
