// hda_mgr.hip -- MGR (multigrid reduction) by dof labels, the preconditioner hypredrive builds in
// hypredrv_MGRCreate (reference src/internal/mgr.c; defaults :1226-1330, name maps :1553-1721, argument
// tree include/internal/mgr.h:132-178).  hypre is not part of the reference tree; this is the published
// method (Ries / Trottenberg / Winter; hypre reference manual "MGR") for the option subset
//   prolongation_type  injection | jacobi | l1-jacobi        restriction_type  injection | jacobi | columped
//   f_relaxation       jacobi | l1-jacobi | amg / ilu on A_FF  g_relaxation      none | hybrid (l1) Gauss-Seidel | ilu (ILU(0))
//   coarse_level_type  rap                                    coarsest_level    BoomerAMG (one V-cycle) | ilu
// -- the same definition the CPU checker of the test suite restates.  PARITY UNPINNED against hypre: the
// reference's MGR outputs need data sets that are not in its tree.
// Row partitions: labels, C/F marks and coarse ids of the ghost columns come through the halo plan of the level's
// operator; R reads the same ghost columns as A; P's ghost columns are the ghost C points; A_c = R (A P) is formed
// by two row-partitioned products (dist_spgemm: the rows of the right factor that the ghost columns name are
// fetched from their owners); the coarsest system goes to the row-partitioned BoomerAMG setup.
//
// Per reduction level the unknowns whose label is in f_labels are F points, the rest C points in their
// relative order.  P = [W; I], R = [Z I] are built by row kernels (sequential sums per row: bit-identical to
// the checker), A_c = R (A P) by the deterministic SpGEMM of the AMG setup.  A cycle is global relaxation,
// F-relaxation (a Jacobi sweep of the whole operator with divisors that vanish on C rows), residual,
// restriction, recursion, prolongation: streaming kernels of the AMG solve.
#include "hda_amg.h"
#include "hda_krylov.h"

#include <algorithm>
#include <cstring>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

__global__ __launch_bounds__(256) void k_mgr_mark(int n, const int *__restrict__ labels, const int *__restrict__ fl, int nfl,
                                                  int *__restrict__ cf, int *__restrict__ cmark)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   bool f = false;
   for (int q = 0; q < nfl; q++) f |= (labels[i] == fl[q]);
   cf[i]    = f ? -1 : 1;
   cmark[i] = f ? 0 : 1;
}

// F rows: a_ii, sum over F columns of |a_ij|, sum over all columns of |a_ij| (column order)
__global__ __launch_bounds__(256) void k_mgr_rowstats(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                      const int *__restrict__ cf, double *__restrict__ dF, double *__restrict__ l1F,
                                                      double *__restrict__ l1all)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   double d = 0.0, a = 0.0, b = 0.0;
   if (cf[i] < 0)
      for (int k = rp[i]; k < rp[i + 1]; k++)
      {
         const int j = cj[k];
         b += fabs(v[k]);
         if (j == i) d = v[k];
         if (cf[j] < 0) a += fabs(v[k]);
      }
   dF[i] = d; l1F[i] = a; l1all[i] = b;
}

// column sums of A_FF through the transpose (rows of T ascend: the order of a sequential pass over A's rows)
__global__ __launch_bounds__(256) void k_mgr_colsum(int ncols, const int *__restrict__ trp, const int *__restrict__ tcj, const double *__restrict__ tv,
                                                    const int *__restrict__ cf, double *__restrict__ csum)
{ // j runs over owned and ghost columns; the rows of T are this rank's rows of A
   const int j = blockIdx.x * 256 + threadIdx.x;
   if (j >= ncols) return;
   double s = 0.0;
   if (cf[j] < 0)
      for (int k = trp[j]; k < trp[j + 1]; k++)
         if (cf[tcj[k]] < 0) s += tv[k];
   csum[j] = s;
}
__global__ __launch_bounds__(256) void k_mgr_i2d(int n, const int *__restrict__ in, double *__restrict__ out)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = (double)in[i];
}
__global__ __launch_bounds__(256) void k_mgr_d2i(int n, const double *__restrict__ in, int *__restrict__ out)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = (int)in[i];
}

__global__ __launch_bounds__(256) void k_mgr_dinvF(int n, const int *__restrict__ cf, const double *__restrict__ d, double *__restrict__ dinv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) dinv[i] = (cf[i] < 0 && d[i] != 0.0) ? 1.0 / d[i] : 0.0;
}

// P = [W; I]: C row -> (cidx, 1); F row -> -a_ij / d_i for its C columns (interp 0: empty)
__global__ __launch_bounds__(256) void k_mgr_P_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const int *__restrict__ cf, int interp,
                                                     int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int c = 0;
   if (cf[i] > 0) c = 1;
   else if (interp != 0)
      for (int k = rp[i]; k < rp[i + 1]; k++) c += (cf[cj[k]] > 0);
   cnt[i] = c;
}
__global__ __launch_bounds__(256) void k_mgr_P_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                    const int *__restrict__ cf, const int *__restrict__ cidx, int interp, const double *__restrict__ d,
                                                    const int *__restrict__ prp, int *__restrict__ pcj, double *__restrict__ pv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int q = prp[i];
   if (cf[i] > 0) { pcj[q] = cidx[i]; pv[q] = 1.0; return; }
   if (interp == 0) return;
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (cf[cj[k]] > 0) { pcj[q] = cidx[cj[k]]; pv[q++] = -v[k] / d[i]; }
}

// R = [Z I]: row of C point i -> -a_ij / d_j for its F columns, 1 at column i, columns ascending (restrict 0: identity only)
__global__ __launch_bounds__(256) void k_mgr_R_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const int *__restrict__ cf,
                                                     const int *__restrict__ cidx, int restrict_type, int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] < 0) return;
   int c = 1;
   if (restrict_type != 0)
      for (int k = rp[i]; k < rp[i + 1]; k++) c += (cf[cj[k]] < 0);
   cnt[cidx[i]] = c;
}
__global__ __launch_bounds__(256) void k_mgr_R_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                    const int *__restrict__ cf, const int *__restrict__ cidx, int restrict_type,
                                                    const double *__restrict__ d, const int *__restrict__ rrp, int *__restrict__ rcj,
                                                    double *__restrict__ rv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] < 0) return;
   int  q      = rrp[cidx[i]];
   bool placed = false;
   if (restrict_type != 0)
      for (int k = rp[i]; k < rp[i + 1]; k++)
      {
         const int j = cj[k];
         if (cf[j] > 0) continue;
         if (!placed && j > i) { rcj[q] = i; rv[q++] = 1.0; placed = true; }
         rcj[q] = j;
         rv[q++] = -v[k] / d[j];
      }
   if (!placed) { rcj[q] = i; rv[q] = 1.0; }
}

__global__ __launch_bounds__(256) void k_mgr_coarse_labels(int n, const int *__restrict__ cf, const int *__restrict__ cidx, const int *__restrict__ labels,
                                                           int *__restrict__ lc)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && cf[i] > 0) lc[cidx[i]] = labels[i];
}

__global__ __launch_bounds__(256) void k_iota_add(int n, const int *__restrict__ in, int by, int *__restrict__ out)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = in[i] + by;
}
// global coarse id of the owned C points (as doubles, for the halo exchange)
__global__ __launch_bounds__(256) void k_mgr_cgid(int n, const int *__restrict__ cf, const int *__restrict__ cidx, double first, double *__restrict__ out)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = cf[i] > 0 ? first + (double)cidx[i] : -1.0;
}

// A_FF: rows = owned F points in order, columns = F points (owned: their F index; ghost: fidx holds nf + rank)
__global__ __launch_bounds__(256) void k_mgr_ff_count(int n, const int *__restrict__ rp, const int *__restrict__ cj, const int *__restrict__ cf,
                                                      const int *__restrict__ fidx, int *__restrict__ cnt)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] > 0) return;
   int c = 0;
   for (int k = rp[i]; k < rp[i + 1]; k++) c += (cf[cj[k]] < 0);
   cnt[fidx[i]] = c;
}
__global__ __launch_bounds__(256) void k_mgr_ff_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                     const int *__restrict__ cf, const int *__restrict__ fidx, const int *__restrict__ frp,
                                                     int *__restrict__ fcj, double *__restrict__ fv)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n || cf[i] > 0) return;
   int q = frp[fidx[i]];
   for (int k = rp[i]; k < rp[i + 1]; k++)
      if (cf[cj[k]] < 0) { fcj[q] = fidx[cj[k]]; fv[q++] = v[k]; }
}
__global__ __launch_bounds__(256) void k_mgr_gatherF(int n, const int *__restrict__ cf, const int *__restrict__ fidx, const double *__restrict__ t,
                                                     double *__restrict__ rF)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && cf[i] < 0) rF[fidx[i]] = t[i];
}
__global__ __launch_bounds__(256) void k_mgr_addF(int n, const int *__restrict__ cf, const int *__restrict__ fidx, const double *__restrict__ eF, double *u)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n && cf[i] < 0) u[i] += eF[fidx[i]];
}
__global__ __launch_bounds__(256) void k_mgr_fmark(int n, const int *__restrict__ cf, int *__restrict__ fm)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) fm[i] = cf[i] < 0 ? 1 : 0;
}

bool gs_type(int t) { return t == 3 || t == 4 || t == 6 || t == 8 || t == 13 || t == 14 || t == 88; }

void finish_csr(DCsr &M, int nrows, int ncols, DArray<int> &cnt)
{
   M.nrows = nrows;
   M.ncols = ncols;
   M.rowptr.alloc((size_t)nrows + 1);
   require_int32_total(nrows, cnt.data(), "MGR transfer operator");
   exclusive_scan(nrows, cnt.data(), M.rowptr.data(), nullptr);
   HDA_HIP(hipMemcpyAsync(&M.nnz, M.rowptr.data() + nrows, 4, hipMemcpyDeviceToHost, STREAM));
   Context::get().sync();
   M.col.alloc((size_t)std::max(M.nnz, 1));
   M.val.alloc((size_t)std::max(M.nnz, 1));
}

} // namespace

void Mgr::setup(const DCsr &A0, const std::vector<int> &labels0)
{
   HDA_REQUIRE(Comm::world().size == 1, "MGR: a row-partitioned matrix needs setup_dist");
   std::vector<long long> part = {0, (long long)A0.nrows}, ghosts;
   setup_dist(A0, hA0_none, part, ghosts, labels0);
}

void Mgr::setup_dist(const DCsr &A0, const HaloPlan &hA0, const std::vector<long long> &part0, const std::vector<long long> &ghosts0,
                     const std::vector<int> &labels0)
{
   Comm      &cm    = Comm::world();
   const bool multi = cm.size > 1;
   HDA_REQUIRE((int)labels0.size() == A0.nrows, "MGR: the dofmap must label every local row");
   HDA_REQUIRE(!prm.levels.empty(), "MGR: at least one reduction level (preconditioner.mgr.level.0.f_dofs) is needed");
   HDA_REQUIRE(A0.ncols == A0.nrows + (int)ghosts0.size(), "MGR: ghost list does not match the matrix block");
   lv.clear();
   lv.resize(prm.levels.size());
   a0_dims[0] = A0.nrows; a0_dims[1] = A0.ncols; a0_dims[2] = A0.nnz;
   const DCsr             *A  = &A0;
   const HaloPlan         *hA = &hA0;
   std::vector<long long>  part = part0, ghosts = ghosts0;
   DArray<int>             labels;
   labels.upload(labels0.data(), std::max<size_t>(labels0.size(), 1));
   level_ms.assign(prm.levels.size() + 1, 0.0);
   for (size_t l = 0; l < prm.levels.size(); l++)
   {
      const auto            t0 = std::chrono::steady_clock::now();
      const MgrLevelParams &p = prm.levels[l];
      Level                &L = lv[l];
      HDA_REQUIRE(p.interp_type == 0 || p.interp_type == 1 || p.interp_type == 2 || p.interp_type == 12,
                  "MGR prolongation_type: injection, jacobi, l1-jacobi and blk-jacobi are implemented");
      HDA_REQUIRE(p.restrict_type == 0 || p.restrict_type == 2 || p.restrict_type == 14,
                  "MGR restriction_type: injection, jacobi and columped are implemented");
      HDA_REQUIRE(p.coarse_type == 0 || p.coarse_type == 1, "MGR coarse_level_type: rap (Galerkin) and non-galerkin are implemented");
      HDA_REQUIRE(p.coarse_th >= 0.0, "MGR coarse_th must not be negative");
      HDA_REQUIRE(p.frelax_type == 7 || p.frelax_type == 18 || p.frelax_type == 2 || p.frelax_type == 32,
                  "MGR f_relaxation: jacobi (single), l1-jacobi, amg and ilu are implemented");
      HDA_REQUIRE(p.grelax_type < 0 || gs_type(p.grelax_type) || p.grelax_type == 16,
                  "MGR g_relaxation: none, the hybrid (l1) Gauss-Seidel types and ilu are implemented");
      HDA_REQUIRE(!p.f_labels.empty(), "MGR: a reduction level without f_dofs");
      const int n = A->nrows, nx = A->ncols, ng = nx - n; // owned rows, owned + ghost columns
      L.A  = A;
      L.hA = hA;
      L.n  = n;
      // labels of the ghost columns, then C/F marks of owned and ghost unknowns
      DArray<double> dtmp((size_t)std::max(nx, 1));
      L.labels.alloc((size_t)std::max(nx, 1));
      if (n) k_mgr_i2d<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, labels.data(), dtmp.data());
      if (multi) halo_exchange(*hA, dtmp.data());
      if (nx) k_mgr_d2i<<<ceil_div(nx, 256), 256, 0, STREAM>>>(nx, dtmp.data(), L.labels.data());
      L.cf.alloc((size_t)std::max(nx, 1));
      DArray<int> fl, cmark((size_t)nx + 1), cscan((size_t)nx + 1);
      fl.upload(p.f_labels.data(), p.f_labels.size());
      cmark.zero();
      if (nx) k_mgr_mark<<<ceil_div(nx, 256), 256, 0, STREAM>>>(nx, L.labels.data(), fl.data(), (int)p.f_labels.size(), L.cf.data(), cmark.data());
      // coarse numbering: owned C points 0..nc-1 in order; ghost C points nc + their rank among the ghost C points
      // (ghosts ascend by global id, so do their coarse ids)
      int nc = 0, ncx = 0;
      exclusive_scan(n, cmark.data(), cscan.data(), nullptr);
      HDA_HIP(hipMemcpyAsync(&nc, cscan.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
      Context::get().sync();
      L.cidx.alloc((size_t)nx + 1);
      L.cidx.copy_from(cscan);
      if (ng)
      {
         DArray<int> gscan((size_t)ng + 1);
         exclusive_scan(ng, cmark.data() + n, gscan.data(), nullptr);
         k_iota_add<<<ceil_div(ng, 256), 256, 0, STREAM>>>(ng, gscan.data(), nc, L.cidx.data() + n);
         HDA_HIP(hipMemcpyAsync(&ncx, gscan.data() + ng, 4, hipMemcpyDeviceToHost, STREAM));
         Context::get().sync();
      }
      L.nc = nc;
      L.row0 = part[(size_t)cm.rank];
      L.aghosts = ghosts;
      // coarse row starts of every rank, global coarse ids of the ghost C points
      std::vector<long long> cpart((size_t)cm.size + 1, 0);
      {
         std::vector<long long> all;
         cm.allgather_ll(nc, all);
         for (int r = 0; r < cm.size; r++) cpart[(size_t)r + 1] = cpart[(size_t)r] + all[(size_t)r];
      }
      long long tot[2] = {nc, n};
      cm.allreduce_host(tot, 2, 0);
      HDA_REQUIRE(tot[0] > 0 && tot[0] < tot[1], "MGR: a reduction level must keep some unknowns and eliminate some (check f_dofs against the dofmap labels)");
      std::vector<long long> pghosts; // coarse ids of P's ghost columns
      if (multi)
      {
         DArray<double> cg((size_t)std::max(nx, 1));
         k_mgr_cgid<<<ceil_div(std::max(n, 1), 256), 256, 0, STREAM>>>(n, L.cf.data(), L.cidx.data(), (double)cpart[(size_t)cm.rank], cg.data());
         halo_exchange(*hA, cg.data());
         std::vector<double> hg((size_t)std::max(ng, 1));
         std::vector<int>    hcf((size_t)std::max(ng, 1));
         if (ng)
         {
            HDA_HIP(hipMemcpyAsync(hg.data(), cg.data() + n, 8 * (size_t)ng, hipMemcpyDeviceToHost, STREAM));
            HDA_HIP(hipMemcpyAsync(hcf.data(), L.cf.data() + n, 4 * (size_t)ng, hipMemcpyDeviceToHost, STREAM));
            Context::get().sync();
         }
         for (int g = 0; g < ng; g++)
            if (hcf[(size_t)g] > 0) pghosts.push_back((long long)hg[(size_t)g]);
         HDA_REQUIRE((int)pghosts.size() == ncx, "MGR: ghost coarse numbering is inconsistent");
      }
      L.c0      = cpart[(size_t)cm.rank];
      L.pghosts = pghosts;
      // row statistics of the F rows (ghost F columns see their owners' values), column sums of A_FF
      DArray<double> dF((size_t)std::max(nx, 1)), l1F((size_t)std::max(nx, 1)), l1all((size_t)std::max(nx, 1)), csum;
      dF.zero();
      if (n)
         k_mgr_rowstats<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), A->val.data(), L.cf.data(), dF.data(), l1F.data(),
                                                             l1all.data());
      if (multi && p.restrict_type == 2) halo_exchange(*hA, dF.data());
      if (p.restrict_type == 14)
      {
         DCsr T;
         transpose(*A, T);
         csum.alloc((size_t)std::max(nx, 1));
         if (nx) k_mgr_colsum<<<ceil_div(nx, 256), 256, 0, STREAM>>>(nx, T.rowptr.data(), T.col.data(), T.val.data(), L.cf.data(), csum.data());
         if (multi)
         {
            halo_reverse_add(*hA, csum.data()); // contributions of the rows other ranks own
            halo_exchange(*hA, csum.data());
         }
         Context::get().sync();
      }
      L.dinvF.alloc((size_t)std::max(n, 1));
      if (n) k_mgr_dinvF<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, L.cf.data(), p.frelax_type == 18 ? l1all.data() : dF.data(), L.dinvF.data());
      // F blocks and their inverses (prolongation blk-jacobi, coarse non-galerkin); W_B built once when P is blk-jacobi
      const bool need_blk = p.interp_type == 12 || p.coarse_type == 1;
      DCsr       PB; // P_B = [W_B; I] of a non-Galerkin level whose P is not blk-jacobi
      L.blk = MgrBlocks();
      if (need_blk)
      {
         mgr_blk_build(*A, L.cf.data(), (int)p.f_labels.size(), (int)l, L.row0, 0, L.blk);
         if (p.interp_type != 12) mgr_blk_prolongation(*A, L.cf.data(), L.cidx.data(), nc + ncx, L.blk, PB);
      }
      // P (columns [owned coarse | ghost coarse])
      if (p.interp_type == 12)
      {
         mgr_blk_prolongation(*A, L.cf.data(), L.cidx.data(), nc + ncx, L.blk, L.P);
         if (multi) L.hP = make_halo_plan(nc, cpart, pghosts);
      }
      else
      {
         DArray<int> cnt((size_t)n + 1);
         cnt.zero();
         if (n) k_mgr_P_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), L.cf.data(), p.interp_type, cnt.data());
         finish_csr(L.P, n, nc + ncx, cnt);
         if (n)
            k_mgr_P_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), A->val.data(), L.cf.data(), L.cidx.data(), p.interp_type,
                                                              p.interp_type == 1 ? l1F.data() : dF.data(), L.P.rowptr.data(), L.P.col.data(),
                                                              L.P.val.data());
         if (multi) L.hP = make_halo_plan(nc, cpart, pghosts);
      }
      // R (columns = the fine columns of A, ghosts included)
      {
         DArray<int> cnt((size_t)nc + 1);
         cnt.zero();
         if (n) k_mgr_R_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), L.cf.data(), L.cidx.data(), p.restrict_type, cnt.data());
         finish_csr(L.R, nc, nx, cnt);
         if (n)
            k_mgr_R_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), A->val.data(), L.cf.data(), L.cidx.data(), p.restrict_type,
                                                              p.restrict_type == 14 ? csum.data() : dF.data(), L.R.rowptr.data(), L.R.col.data(),
                                                              L.R.val.data());
      }
      // f_relaxation amg: A_FF in the relative order of the F points and a BoomerAMG hierarchy on it
      if (p.frelax_type == 2 || p.frelax_type == 32)
      {
         DArray<int> fm((size_t)nx + 1), fs((size_t)nx + 1);
         fm.zero();
         if (nx) k_mgr_fmark<<<ceil_div(nx, 256), 256, 0, STREAM>>>(nx, L.cf.data(), fm.data());
         exclusive_scan(n, fm.data(), fs.data(), nullptr);
         int nf = 0, nfx = 0;
         HDA_HIP(hipMemcpyAsync(&nf, fs.data() + n, 4, hipMemcpyDeviceToHost, STREAM));
         Context::get().sync();
         L.fidx.alloc((size_t)nx + 1);
         L.fidx.copy_from(fs);
         if (ng)
         {
            DArray<int> gs((size_t)ng + 1);
            exclusive_scan(ng, fm.data() + n, gs.data(), nullptr);
            k_iota_add<<<ceil_div(ng, 256), 256, 0, STREAM>>>(ng, gs.data(), nf, L.fidx.data() + n);
            HDA_HIP(hipMemcpyAsync(&nfx, gs.data() + ng, 4, hipMemcpyDeviceToHost, STREAM));
            Context::get().sync();
         }
         L.nf = nf;
         L.fpart.assign((size_t)cm.size + 1, 0);
         {
            std::vector<long long> all;
            cm.allgather_ll(nf, all);
            for (int r = 0; r < cm.size; r++) L.fpart[(size_t)r + 1] = L.fpart[(size_t)r] + all[(size_t)r];
         }
         L.fghosts.clear();
         if (multi)
         { // global F ids of the ghost F columns (ascending with the ghosts' global ids)
            DArray<double> fg((size_t)std::max(nx, 1));
            k_mgr_cgid<<<ceil_div(std::max(n, 1), 256), 256, 0, STREAM>>>(n, fm.data(), L.fidx.data(), (double)L.fpart[(size_t)cm.rank], fg.data());
            halo_exchange(*hA, fg.data());
            std::vector<double> hg((size_t)std::max(ng, 1));
            std::vector<int>    hcf((size_t)std::max(ng, 1));
            if (ng)
            {
               HDA_HIP(hipMemcpyAsync(hg.data(), fg.data() + n, 8 * (size_t)ng, hipMemcpyDeviceToHost, STREAM));
               HDA_HIP(hipMemcpyAsync(hcf.data(), L.cf.data() + n, 4 * (size_t)ng, hipMemcpyDeviceToHost, STREAM));
               Context::get().sync();
            }
            for (int g = 0; g < ng; g++)
               if (hcf[(size_t)g] < 0) L.fghosts.push_back((long long)hg[(size_t)g]);
            HDA_REQUIRE((int)L.fghosts.size() == nfx, "MGR: ghost F numbering is inconsistent");
         }
         DArray<int> cnt((size_t)nf + 1);
         cnt.zero();
         if (n) k_mgr_ff_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), L.cf.data(), L.fidx.data(), cnt.data());
         finish_csr(L.Aff, nf, nf + nfx, cnt);
         if (n)
            k_mgr_ff_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, A->rowptr.data(), A->col.data(), A->val.data(), L.cf.data(), L.fidx.data(),
                                                               L.Aff.rowptr.data(), L.Aff.col.data(), L.Aff.val.data());
         sort_rows(L.Aff); // ghosts below the owned range sort after the owned columns in the block layout
         size_t fl = (size_t)std::max(L.Aff.ncols, 1);
         if (p.frelax_type == 32)
         { // block-Jacobi ILU(0) of this rank's diagonal block of A_FF
            L.filu = std::make_unique<Ilu>();
            L.filu->setup(L.Aff, p.ilu);
            if (multi && p.fkrylov_method >= 0) L.hFF = make_halo_plan(nf, L.fpart, L.fghosts); // the nested solve's products need it
         }
         else
         {
            AmgParams fp = p.frelax_amg;
            fp.max_iter  = 1;
            L.famg       = std::make_unique<Amg>(fp);
            if (multi)
            {
               L.hFF = make_halo_plan(nf, L.fpart, L.fghosts);
               const char *mode = getenv("HDA_DIST_SETUP");
               L.famg->dof_row_offset = L.fpart[(size_t)cm.rank]; // systems AMG: function = global A_FF index mod num_functions
               if ((mode && !strcmp(mode, "replicated")) || fp.coarsen_type != 8 || fp.num_functions > 1) L.famg->setup_dist(L.Aff, L.hFF, L.fpart, L.fghosts);
               else L.famg->setup_dist_partitioned(L.Aff, L.hFF, L.fpart, L.fghosts);
            }
            else L.famg->setup(L.Aff);
            fl = std::max(fl, L.famg->vec_len0());
         }
         L.rF.alloc(fl);
         L.eF.alloc(fl);
      }
      // global relaxation data
      if (p.grelax_type == 16)
      { // hypre's default ILU as global smoother: block-Jacobi ILU(0), exact triangular solves
         L.gilu = std::make_unique<Ilu>();
         IluParams ip = p.ilu;
         ip.max_iter  = std::max(p.grelax_sweeps, 1);
         L.gilu->setup(*A, ip);
      }
      else if (p.grelax_type >= 0)
      {
         DArray<double> d((size_t)std::max(n, 1));
         const int      t = p.grelax_type == 88 ? 8 : p.grelax_type;
         // Row blocks (MgrLevelParams::grelax_blocks, as AmgParams::blocks): hypre's hybrid sweep is Gauss-Seidel over a RANK's rows, so V
         // contiguous blocks on one GPU are what the reference computes at np = V; one block is the sequential sweep (np = 1), level
         // scheduled -- 2 n^(1/2) .. 3 n^(1/3) launches per sweep, which is what bound BASELINE config 4's stand-in (round 5: 39 ms per
         // solve at 786 k rows, the level-0 product 0.02 ms).  0 = the setup's choice, announced like BoomerAMG's.
         int V = multi ? 1 : p.grelax_blocks;
         if (V == 0) V = amg_auto_blocks(*A);
         if (V > 1 && n >= V)
         {
            std::vector<int> part((size_t)V + 1);
            for (int q = 0; q <= V; q++) part[(size_t)q] = (int)(((long long)q * n) / V); // hypre_GeneratePartitioning
            build_gs_plan_blocks(*A, part, L.gs);
            if (t == 8 || t == 13 || t == 14) l1_row_norms(*A, 4, d.data(), L.gs.blk_part.data(), V);
            else extract_diag(*A, d.data());
            if (p.grelax_blocks == 0 && !getenv("HDA_QUIET"))
               fprintf(stderr, "[hypredrv_amd] MGR setup, level %d: %d row blocks of about %d rows chosen by the setup: the hybrid Gauss-Seidel global relaxation "
                               "runs as the reference computes it on %d ranks (HDA_BLOCKS=1: one block, the np = 1 sweep)\n", (int)l, V, n / V, V);
         }
         else
         {
            if (t == 8 || t == 13 || t == 14) l1_row_norms(*A, 4, d.data());
            else extract_diag(*A, d.data());
            build_gs_plan(*A, L.gs);
         }
         L.dinvG.alloc((size_t)std::max(n, 1));
         make_dinv(n, d.data(), 1.0, L.dinvG.data());
      }
      // coarse operator A_c = R (A P), its ghost list and halo plan, the labels of its rows
      Level                  *next = (l + 1 < prm.levels.size()) ? &lv[l + 1] : nullptr;
      DCsr                   &Anext = next ? next->A_own : Ac;
      std::vector<long long>  cghosts;
      if (p.coarse_type == 1)
      { // non-Galerkin: A_c = A_CC + Ahat_CF W_B = M P_B (M: the C rows of A with their F entries cut)
         std::vector<long long> gids((size_t)std::max(nx, 1));
         for (int j = 0; j < n; j++) gids[(size_t)j] = L.row0 + j;
         for (int g = 0; g < ng; g++) gids[(size_t)(n + g)] = ghosts[(size_t)g];
         DCsr        M;
         const DCsr &PBr = p.interp_type == 12 ? L.P : PB;
         mgr_nongalerkin_rows(*A, L.cf.data(), L.cidx.data(), nc, gids, p.nonglk_max_elmts, M);
         if (multi) dist_spgemm(M, *hA, PBr, pghosts, cpart, Anext, cghosts);
         else spgemm(M, PBr, Anext);
      }
      else if (multi)
      {
         DCsr                   AP;
         std::vector<long long> apg;
         dist_spgemm(*A, *hA, L.P, pghosts, cpart, AP, apg);
         dist_spgemm(L.R, *hA, AP, apg, cpart, Anext, cghosts);
      }
      else
      {
         DCsr AP;
         spgemm(*A, L.P, AP);
         spgemm(L.R, AP, Anext);
      }
      if (p.coarse_th > 0.0) mgr_coarse_drop(Anext, p.coarse_th, multi ? &cghosts : nullptr);
      DArray<int> lc((size_t)std::max(nc, 1));
      if (n) k_mgr_coarse_labels<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, L.cf.data(), L.cidx.data(), L.labels.data(), lc.data());
      Context::get().sync();
      HaloPlan &hnext = next ? next->hA_own : hAc;
      if (multi) hnext = make_halo_plan(nc, cpart, cghosts);
      // work vectors: every one may carry the ghost tail of A, of P (on the coarse side) or of A_c
      const size_t len = (size_t)std::max(std::max(nx, n), 1);
      if (l > 0) { L.f.alloc(std::max(len, L.flen)); L.u.alloc(std::max(len, L.flen)); }
      L.u2.alloc(std::max(len, L.flen)); // the cycle may hand u2 back to the finer level, whose P reads its own ghost tail in it
      L.t.alloc(len);
      const size_t clen = (size_t)std::max(std::max(Anext.ncols, L.P.ncols), 1);
      if (next) next->flen = clen;
      else coarse_len = clen;
      spmv_prepare(*A);
      spmv_prepare(L.P);
      spmv_prepare(L.R);
      if (!prm.keep_blocks) L.blk = MgrBlocks(); // P and A_c are built: the inverses are only kept for the test entry
      labels = std::move(lc);
      A      = &Anext;
      hA     = &hnext;
      part   = cpart;
      ghosts = cghosts;
      Context::get().sync();
      level_ms[l] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
   }
   const auto tc = std::chrono::steady_clock::now();
   auto coarse_time = [&] { level_ms.back() = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count(); };
   cparts  = part;
   cghosts_ = ghosts;
   // coarsest system: BoomerAMG, or block-Jacobi ILU(0) iterations
   if (prm.coarse_is_ilu)
   {
      camg.reset();
      cilu = std::make_unique<Ilu>();
      cilu->setup(Ac, prm.coarse_ilu);
      const size_t clen = std::max(coarse_len, (size_t)std::max(Ac.ncols, 1));
      fc.alloc(clen);
      uc.alloc(clen);
      Context::get().sync();
      coarse_time();
      return;
   }
   cilu.reset();
   camg = std::make_unique<Amg>(prm.coarse);
   if (multi)
   {
      const char *mode = getenv("HDA_DIST_SETUP");
      if ((mode && !strcmp(mode, "replicated")) || prm.coarse.coarsen_type != 8 || prm.coarse.num_functions > 1) camg->setup_dist(Ac, hAc, cparts, cghosts_);
      else camg->setup_dist_partitioned(Ac, hAc, cparts, cghosts_);
   }
   else camg->setup(Ac);
   const size_t clen = std::max<size_t>(std::max(camg->vec_len0(), coarse_len), (size_t)std::max(Ac.ncols, 1));
   fc.alloc(clen);
   uc.alloc(clen);
   Context::get().sync();
   coarse_time();
}

void Mgr::dist_view(int level, int which, long long &row0, long long &col0, std::vector<long long> &ghosts) const
{
   HDA_REQUIRE(level >= 0 && level <= (int)lv.size() && (which == 0 || which == 1) && !(which == 1 && level == (int)lv.size()), "MGR view out of range");
   if (level == (int)lv.size())
   {
      row0 = col0 = cparts[(size_t)Comm::world().rank];
      ghosts = cghosts_;
      return;
   }
   const Level &L = lv[(size_t)level];
   row0   = L.row0;
   col0   = which == 0 ? L.row0 : L.c0;
   ghosts = which == 0 ? L.aghosts : L.pghosts;
}

std::vector<double> Mgr::block_inverses(int level, int tier, int &b, int &nf)
{
   HDA_REQUIRE(level >= 0 && level < (int)lv.size(), "MGR level out of range");
   HDA_REQUIRE(tier >= 0 && tier <= 2, "MGR block inverses: tier 0 (the setup's), 1 (b <= 8) or 2");
   Level &L = lv[(size_t)level];
   b        = L.blk.b;
   nf       = L.blk.nf;
   HDA_REQUIRE(b > 0 || prm.keep_blocks || (prm.levels[(size_t)level].interp_type != 12 && prm.levels[(size_t)level].coarse_type != 1),
               "MGR block inverses: this handle did not keep them (MgrParams::keep_blocks)");
   if (b == 0) return {};
   if (tier > 0)
   {
      MgrBlocks T;
      T.b = L.blk.b; T.nf = L.blk.nf; T.nblk = L.blk.nblk;
      T.fidx.copy_from(L.blk.fidx);
      T.frow.copy_from(L.blk.frow);
      mgr_blk_invert(*L.A, L.cf.data(), level, L.row0, tier, T);
      return T.inv.to_host();
   }
   return L.blk.inv.to_host();
}

void Mgr::rebind(const DCsr &A, const HaloPlan *hA)
{
   HDA_REQUIRE(!lv.empty(), "rebind before setup");
   HDA_REQUIRE(A.nrows == a0_dims[0] && A.ncols == a0_dims[1],
               "a reused MGR preconditioner needs a matrix with the same local rows and ghost layer as the one it was built for");
   lv[0].A = &A;
   if (hA) lv[0].hA = hA;
   a0_dims[2] = A.nnz;
   spmv_prepare(A);
}

const DCsr &Mgr::matrix(int level, int which) const
{
   HDA_REQUIRE(level >= 0 && level <= (int)lv.size(), "MGR level out of range");
   if (level == (int)lv.size())
   {
      HDA_REQUIRE(which == 0, "the coarsest MGR level has no transfer operators");
      return Ac;
   }
   const Level &L = lv[(size_t)level];
   return which == 0 ? *L.A : which == 1 ? L.P : L.R;
}

// A nested Krylov component (reference src/internal/krylov.c:557-603): the solver runs to its own max_iter / tolerance from the
// guess it is given; not reaching the tolerance is no error (it is an inexact smoother / coarse solve).
static void nested_krylov(int method, const NestedKrylov &k, const LinOp &op, const PrecondFn &M, const double *b, double *x)
{
   KrylovParams kp;
   kp.max_iter = k.max_iter; kp.rtol = k.rtol; kp.atol = k.atol; kp.krylov_dim = k.krylov_dim; kp.min_iter = k.min_iter;
   kp.two_norm = k.two_norm; kp.skip_real_res_check = k.skip_real_res_check; kp.print_level = 0;
   switch (method)
   {
      case 0: pcg(op, M, kp, b, x); break;
      case 1: gmres(op, M, kp, b, x); break;
      case 2: fgmres(op, M, kp, b, x); break;
      case 3: bicgstab(op, M, kp, b, x); break;
      default: HDA_REQUIRE(false, "MGR: unknown nested Krylov method");
   }
}

// one cycle on level l: u holds the current iterate (zero = it is known to be zero); returns where the result lives
double *Mgr::cycle(int l, const double *f, double *u, bool zero)
{
   if (l == (int)lv.size())
   {
      const bool multi = Comm::world().size > 1;
      if (prm.ckrylov_method >= 0)
      {
         fill((int)uc.size(), 0.0, u);
         PrecondFn M;
         if (prm.ckrylov_precond && camg) M = [this](const double *r, double *z, int slot) { camg->apply(r, z, -1); if (slot >= 0) dot(Ac.nrows, r, z, slot); };
         else if (prm.ckrylov_precond && cilu)
            M = [this, multi](const double *r, double *z, int slot) {
               stationary_solve(*cilu, Ac, multi ? &hAc : nullptr, r, z, true, std::max(cilu->prm.max_iter, 1), cilu_r, cilu_c);
               if (slot >= 0) dot(Ac.nrows, r, z, slot);
            };
         nested_krylov(prm.ckrylov_method, prm.ckrylov, LinOp(Ac, multi ? &hAc : nullptr, uc.size()), M, f, u);
      }
      else if (camg) camg->apply(f, u, -1);
      else stationary_solve(*cilu, Ac, multi ? &hAc : nullptr, f, u, true, std::max(cilu->prm.max_iter, 1), cilu_r, cilu_c);
      return u;
   }
   Level                &L = lv[(size_t)l];
   const MgrLevelParams &p = prm.levels[(size_t)l];
   const DCsr           &A = *L.A;
   const int             n = L.n;
   const bool            multi = Comm::world().size > 1;
   double               *cur = u, *alt = L.u2.data();
   auto refresh = [&](double *v) { if (multi) halo_exchange(*L.hA, v); };
   // g_relaxation: sweeps over all points of the level
   auto global_relax = [&]() {
      if (p.grelax_type == 16)
      {
         stationary_solve(*L.gilu, A, multi ? L.hA : nullptr, f, cur, zero, std::max(L.gilu->prm.max_iter, 1), L.ilu_r, L.ilu_c);
         zero = false;
      }
      else if (p.grelax_type >= 0)
      {
         const int t = p.grelax_type;
         if (L.gs.nblk > 0)
         { // row blocks (one rank): out of place, the other blocks' values are those of the sweep's start; from a zero guess nothing is read
            for (int s = 0; s < std::max(p.grelax_sweeps, 1); s++)
               for (int dir = 0; dir < 2; dir++)
               {
                  const bool fwd = dir == 0;
                  if (fwd ? !(t == 3 || t == 13 || t == 6 || t == 8 || t == 88) : !(t == 4 || t == 14 || t == 6 || t == 8 || t == 88)) continue;
                  if (zero) gs_sweep_blocks(A, L.gs, L.dinvG.data(), f, nullptr, cur, fwd, true);
                  else { gs_sweep_blocks(A, L.gs, L.dinvG.data(), f, cur, alt, fwd, false); std::swap(cur, alt); }
                  zero = false;
               }
            return;
         }
         if (zero) fill((int)std::max(A.ncols, n), 0.0, cur);
         zero = false;
         for (int s = 0; s < std::max(p.grelax_sweeps, 1); s++)
         {
            if (t == 3 || t == 13 || t == 6 || t == 8 || t == 88) { refresh(cur); gs_sweep(A, L.gs, L.dinvG.data(), f, cur, true); }
            if (t == 4 || t == 14 || t == 6 || t == 8 || t == 88) { refresh(cur); gs_sweep(A, L.gs, L.dinvG.data(), f, cur, false); }
         }
      }
   };
   // f_relaxation: sweeps on the F points of the level
   auto f_relax = [&]() {
      for (int s = 0; s < p.frelax_sweeps; s++)
      {
         if (p.frelax_type == 2 || p.frelax_type == 32)
         { // e_F = M_FF^-1 (f - A u)_F (one BoomerAMG cycle from a zero guess, or one ILU(0) solve), u_F += e_F
            if (zero) { fill((int)std::max(A.ncols, n), 0.0, cur); zero = false; }
            refresh(cur);
            residual(A, cur, f, L.t.data());
            if (n) k_mgr_gatherF<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, L.cf.data(), L.fidx.data(), L.t.data(), L.rF.data());
            if (p.fkrylov_method >= 0)
            { // nested Krylov solve of A_FF e_F = r_F from a zero guess, preconditioned by the level's component
               fill((int)L.eF.size(), 0.0, L.eF.data());
               PrecondFn M;
               // (a PCG caller hands over the slot it wants the block partials of <r, z> in)
               if (p.fkrylov_precond && L.famg) M = [&L](const double *r, double *z, int slot) { L.famg->apply(r, z, -1); if (slot >= 0) dot(L.nf, r, z, slot); };
               else if (p.fkrylov_precond && L.filu) M = [&L](const double *r, double *z, int slot) { L.filu->apply(r, z); if (slot >= 0) dot(L.nf, r, z, slot); };
               nested_krylov(p.fkrylov_method, p.fkrylov, LinOp(L.Aff, multi ? &L.hFF : nullptr, L.eF.size()), M, L.rF.data(), L.eF.data());
            }
            else if (L.famg) L.famg->apply(L.rF.data(), L.eF.data(), -1);
            else L.filu->apply(L.rF.data(), L.eF.data());
            if (n) k_mgr_addF<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, L.cf.data(), L.fidx.data(), L.eF.data(), cur);
            continue;
         }
         if (zero) { jacobi_zero_guess(n, L.dinvF.data(), f, cur); zero = false; continue; } // u = dinvF .* f
         refresh(cur);
         jacobi(A, L.dinvF.data(), f, cur, alt, -1);
         std::swap(cur, alt);
      }
   };
   // smoothing positions (reference mgr.c:614-675: v(1,0) pre, v(0,1) post, v(1,1) both; hypre's SetGlobalSmoothCycle /
   // SetFRelaxCycle): before the coarse correction global relaxation then F-relaxation, after it the mirror image
   if (prm.gsmooth_pos & 1) global_relax();
   if (prm.frelax_pos & 1) f_relax();
   const bool last = (l + 1 == (int)lv.size());
   double    *fcl  = last ? fc.data() : lv[(size_t)l + 1].f.data();
   double    *ucl  = last ? uc.data() : lv[(size_t)l + 1].u.data();
   // W-cycle (cycle 2): the coarser level is visited twice
   for (int visit = 0; visit < (prm.cycle == 2 ? 2 : 1); visit++)
   {
      if (zero) { fill(n, 0.0, cur); zero = false; }
      refresh(cur);
      residual(A, cur, f, L.t.data());
      refresh(L.t.data());
      spmv(L.R, 1.0, L.t.data(), 0.0, nullptr, fcl);
      double *ec = cycle(l + 1, fcl, ucl, true);
      if (multi) halo_exchange(L.hP, ec);
      spmv(L.P, 1.0, ec, 1.0, cur, cur);
   }
   if (prm.frelax_pos & 2) f_relax();
   if (prm.gsmooth_pos & 2) global_relax();
   return cur;
}

void Mgr::solve(const double *b, double *x, bool zero_guess)
{
   const int n = lv.empty() ? 0 : lv[0].n;
   for (int it = 0; it < std::max(prm.max_iter, 1); it++)
   {
      double *r = cycle(0, b, x, zero_guess && it == 0);
      if (r != x) copy(n, r, x);
   }
}

} // namespace hda
