// hda_capi.hip -- kernel-level C ABI (include/hypredrv_amd.h).  Host buffers in / out.
#include "../../include/hypredrv_amd.h"

#include "hda_precond.h"
#include "hda_multi.h"
#include "hda_comm.h"
#include "hda_hypre.h"

#include <chrono>
#include <cmath>
#include <cstring>

using namespace hda;

struct hda_csr_s {
   DCsr           m;
   DArray<double> rhs; // optional device rhs (generator)
   bool           borrowed = false;
   const DCsr    *ref      = nullptr; // for borrowed handles
   const double  *rhs_ref  = nullptr; // device rhs of a handle borrowed from a HYPREDRV object
   const HaloPlan *halo    = nullptr; // its ghost refresh plan (row-partitioned runs)
   const DCsr    &get() const { return ref ? *ref : m; }
};
struct hda_amg_s {
   Precond                                 pc; // what hda_*_create made: a hierarchy (owned, or borrowed from a HYPREDRV object) or one of the other kinds
   hda_csr_t                               A = nullptr;
   std::vector<std::unique_ptr<hda_csr_s>> views;
};

#define g_err (RankState<std::string, 1>::get())

extern "C" const char *hda_last_error(void) { return g_err.c_str(); }

extern "C" int hda_device_count(void)
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

#define HDA_TRY                           \
   try                                    \
   {                                      \
      if (hda_device_count() < 1)         \
      {                                   \
         g_err = "no HIP device visible: the MI355X solve path has no CPU fallback"; \
         return HDA_ERR_NO_DEVICE;        \
      }
#define HDA_CATCH                         \
   }                                      \
   catch (const std::exception &e)        \
   {                                      \
      g_err = e.what();                   \
      return HDA_ERR_RUNTIME;             \
   }                                      \
   return HDA_OK;

extern "C" int hda_device_name(char *buf, int len)
{
   HDA_TRY
   hipDeviceProp_t p;
   HDA_HIP(hipGetDeviceProperties(&p, Context::get().device));
   snprintf(buf, (size_t)len, "%s (%s), %d CUs", p.name, p.gcnArchName, p.multiProcessorCount);
   HDA_CATCH
}

// PCI bus id of visible device `dev` ("0000:c1:00.0"): the identity of the physical GPU, which an index is not once a launcher has
// narrowed every rank's view to its own device (HIP_VISIBLE_DEVICES per rank: all indices are 0).  Touches no context of the library.
extern "C" int hda_device_pci_bus_id(int dev, char *buf, int len)
{
   if (!buf || len < 16) return HDA_ERR_RUNTIME;
   if (hipDeviceGetPCIBusId(buf, len, dev) != hipSuccess)
   {
      (void)hipGetLastError();
      g_err = "hipDeviceGetPCIBusId failed";
      return HDA_ERR_RUNTIME;
   }
   return HDA_OK;
}

extern "C" int hda_device_sync(void)
{
   HDA_TRY
   Context::get().sync();
   HDA_CATCH
}

// a one-thread kernel that does nothing: its name in a kernel trace or counter pass marks a boundary (bench.py brackets its timed
// solves with two of them, tools/pmc_traffic.py sums the counters of the dispatches in between)
__global__ void k_marker(int id, int *sink)
{
   if (id == 0x7fffffff && sink) *sink = id;
}
extern "C" int hda_marker(int id)
{
   HDA_TRY
   k_marker<<<1, 1, 0, Context::get().stream>>>(id, nullptr);
   HDA_CATCH
}

// the C struct of a parameter set: the mirror of to_params below (max_iter, tol and print_level have no field: one cycle, no test)
static void from_params(const AmgParams &d, hda_amg_params *p)
{
   p->coarsen_type = d.coarsen_type; p->interp_type = d.interp_type; p->pmax = d.pmax;
   p->trunc_factor = d.trunc_factor; p->strong_th = d.strong_th; p->max_row_sum = d.max_row_sum;
   p->max_coarse_size = d.max_coarse_size; p->min_coarse_size = d.min_coarse_size; p->max_levels = d.max_levels;
   p->relax_down = d.relax_down; p->relax_up = d.relax_up; p->relax_coarse = d.relax_coarse;
   p->sweeps_down = d.sweeps_down; p->sweeps_up = d.sweeps_up; p->sweeps_coarse = d.sweeps_coarse;
   p->relax_weight = d.relax_weight; p->outer_weight = d.outer_weight; p->seed = d.seed; p->num_functions = d.num_functions;
   p->cheby_order = d.cheby_order; p->cheby_eig_est = d.cheby_eig_est; p->cheby_variant = d.cheby_variant; p->cheby_scale = d.cheby_scale;
   p->cheby_fraction = d.cheby_fraction;
   p->smooth_num_levels = d.smooth_num_levels; p->smooth_num_sweeps = d.smooth_num_sweeps;
   p->ilu_tri_solve = d.ilu.tri_solve; p->ilu_lower_it = d.ilu.lower_it; p->ilu_upper_it = d.ilu.upper_it;
   p->restrict_type = d.restrict_type; p->restrict_strong_th = d.restrict_strong_th; p->restrict_filter_th = d.restrict_filter_th;
   p->relax_points = d.relax_points;
   p->agg_num_levels = d.agg_num_levels; p->agg_num_paths = d.agg_num_paths; p->agg_interp_type = d.agg_interp_type;
   p->agg_pmax = d.agg_pmax; p->agg_trunc_factor = d.agg_trunc_factor;
   p->agg_p12_pmax = d.agg_p12_pmax; p->agg_p12_trunc_factor = d.agg_p12_trunc_factor;
   p->smooth_type = d.smooth_type; p->fsai_num_levels = d.fsai.num_levels; p->fsai_max_nnz_row = d.fsai.max_nnz_row;
   p->fsai_eig_max_iters = d.fsai.eig_max_iters; p->fsai_threshold = d.fsai.threshold;
   p->blocks = d.blocks; p->block_part = nullptr;
   p->struct_size = (int)sizeof(hda_amg_params);
}
extern "C" void hda_amg_default_params(hda_amg_params *p) { from_params(AmgParams(), p); }
extern "C" void hda_krylov_default_params(hda_krylov_params *p, int gmres)
{
   p->max_iter = gmres ? 300 : 100; p->rtol = 1.0e-6; p->atol = 0.0; p->two_norm = 1; p->krylov_dim = 30;
}

static AmgParams to_params(const hda_amg_params *p)
{
   AmgParams a;
   if (!p) return a;
   // a caller compiled against an older, shorter struct passes garbage (or another field) where the size sits
   HDA_REQUIRE(p->struct_size == (int)sizeof(hda_amg_params),
               "hda_amg_params: struct_size does not match this library (start from hda_amg_default_params; rebuild against include/hypredrv_amd.h)");
   a.coarsen_type = p->coarsen_type; a.interp_type = p->interp_type; a.pmax = p->pmax;
   a.trunc_factor = p->trunc_factor; a.strong_th = p->strong_th; a.max_row_sum = p->max_row_sum;
   a.max_coarse_size = p->max_coarse_size; a.min_coarse_size = p->min_coarse_size; a.max_levels = p->max_levels;
   a.relax_down = p->relax_down; a.relax_up = p->relax_up; a.relax_coarse = p->relax_coarse;
   a.sweeps_down = p->sweeps_down; a.sweeps_up = p->sweeps_up; a.sweeps_coarse = p->sweeps_coarse;
   a.relax_weight = p->relax_weight; a.outer_weight = p->outer_weight; a.seed = p->seed;
   a.num_functions = std::max(p->num_functions, 1);
   a.cheby_order = p->cheby_order; a.cheby_eig_est = p->cheby_eig_est; a.cheby_variant = p->cheby_variant; a.cheby_scale = p->cheby_scale;
   a.cheby_fraction = p->cheby_fraction;
   a.smooth_num_levels = p->smooth_num_levels; a.smooth_num_sweeps = p->smooth_num_sweeps;
   a.ilu.tri_solve = p->ilu_tri_solve; a.ilu.lower_it = p->ilu_lower_it; a.ilu.upper_it = p->ilu_upper_it;
   a.restrict_type = p->restrict_type; a.restrict_strong_th = p->restrict_strong_th; a.restrict_filter_th = p->restrict_filter_th;
   a.relax_points = p->relax_points;
   a.agg_num_levels = p->agg_num_levels; a.agg_num_paths = p->agg_num_paths; a.agg_interp_type = p->agg_interp_type;
   a.agg_pmax = p->agg_pmax; a.agg_trunc_factor = p->agg_trunc_factor;
   a.agg_p12_pmax = p->agg_p12_pmax; a.agg_p12_trunc_factor = p->agg_p12_trunc_factor;
   a.smooth_type = p->smooth_type; a.fsai.num_levels = p->fsai_num_levels; a.fsai.max_nnz_row = p->fsai_max_nnz_row;
   a.fsai.eig_max_iters = p->fsai_eig_max_iters; a.fsai.threshold = p->fsai_threshold;
   a.blocks = p->blocks;
   if (p->block_part && p->blocks > 1) a.block_part.assign(p->block_part, p->block_part + p->blocks + 1);
   return a;
}
static std::vector<int> to_part(int nblk, const int64_t *part, int nrows)
{
   HDA_REQUIRE(nblk >= 1 && part, "row blocks: nblk + 1 row starts expected");
   std::vector<int> v((size_t)nblk + 1);
   for (int q = 0; q <= nblk; q++) v[(size_t)q] = (int)part[q];
   HDA_REQUIRE(v.front() == 0 && v.back() == nrows, "row blocks must cover the rows of the operator");
   return v;
}
static KrylovParams to_kparams(const hda_krylov_params *p)
{
   KrylovParams k;
   if (!p) return k;
   k.max_iter = p->max_iter; k.rtol = p->rtol; k.atol = p->atol; k.two_norm = p->two_norm; k.krylov_dim = p->krylov_dim;
   return k;
}

// ---- staging: how every kernel-level entry point below moves host buffers in and out, and hands out matrices
// n host values in a device array of max(n, len, 1) elements: exactly n are read from the caller, whatever lies beyond them is zero
template <class T>
static DArray<T> staged(const T *host, int n, int len = 0)
{
   DArray<T> d((size_t)std::max({n, len, 1}));
   if (d.size() > (size_t)std::max(n, 0)) d.zero();
   if (n > 0) HDA_HIP(hipMemcpyAsync(d.data(), host, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, Context::get().stream));
   Context::get().sync(); // host buffer may be pageable / transient
   return d;
}
// room for n results ...
template <class T>
static DArray<T> room(int n) { return DArray<T>((size_t)std::max(n, 1)); }
// ... and exactly n of them back to the caller
template <class T>
static void fetch(const T *dev, T *host, int n)
{
   if (n > 0) HDA_HIP(hipMemcpyAsync(host, dev, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, Context::get().stream));
   Context::get().sync();
}
// a new matrix, built on the stream, becomes the caller's
static void finish(std::unique_ptr<hda_csr_s> &h, hda_csr_t *out)
{
   Context::get().sync();
   *out = h.release();
}
// a borrowed view of a matrix that lives in the preconditioner of h; the handle keeps the view
static void lend(hda_amg_t h, const DCsr *m, hda_csr_t *out)
{
   auto v      = std::make_unique<hda_csr_s>();
   v->borrowed = true;
   v->ref      = m;
   *out        = v.get();
   h->views.push_back(std::move(v));
}

// ------------------------------------------------------------------ matrices

__global__ void k_cols64_to_32(long nnz, const long long *__restrict__ in, long long offset, int *__restrict__ out)
{
   for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (long)gridDim.x * 256) out[k] = (int)(in[k] - offset);
}

extern "C" int hda_csr_create(int nrows, int ncols, const int64_t *rowptr, const int64_t *cols,
                              const double *vals, hda_csr_t *out)
{
   HDA_TRY
   if (nrows < 0 || ncols < 0 || !out || (nrows > 0 && (!rowptr))) { g_err = "bad argument"; return HDA_ERR_ARG; }
   auto         h    = std::make_unique<hda_csr_s>();
   const int64_t base = nrows ? rowptr[0] : 0;
   const int64_t nnz  = nrows ? rowptr[nrows] - base : 0;
   HDA_REQUIRE(nnz >= 0 && nnz < (1LL << 31), "local nnz must fit int32");
   std::vector<int> rp((size_t)nrows + 1, 0), cj((size_t)nnz);
   for (int i = 0; i <= nrows && nrows; i++) rp[(size_t)i] = (int)(rowptr[i] - base);
   for (int64_t k = 0; k < nnz; k++)
   {
      const int64_t c = cols[base + k];
      HDA_REQUIRE(c >= 0 && c < ncols, "column index out of range");
      cj[(size_t)k] = (int)c;
   }
   h->m.nrows = nrows; h->m.ncols = ncols; h->m.nnz = (int)nnz;
   h->m.rowptr.upload(rp.data(), rp.size());
   h->m.col.alloc((size_t)std::max<int64_t>(nnz, 1));
   h->m.val.alloc((size_t)std::max<int64_t>(nnz, 1));
   if (nnz)
   {
      h->m.col.upload(cj.data(), (size_t)nnz);
      h->m.val.upload(vals + base, (size_t)nnz);
   }
   sort_rows(h->m);
   finish(h, out);
   HDA_CATCH
}

extern "C" int hda_csr_destroy(hda_csr_t A)
{
   if (!A) return HDA_OK;
   try { if (hda_device_count() > 0) Context::get().sync(); } catch (...) {}
   delete A;
   return HDA_OK;
}

extern "C" int hda_csr_dims(hda_csr_t A, int *nrows, int *ncols, int *nnz)
{
   if (!A) { g_err = "null matrix"; return HDA_ERR_ARG; }
   if (nrows) *nrows = A->get().nrows;
   if (ncols) *ncols = A->get().ncols;
   if (nnz) *nnz = A->get().nnz;
   return HDA_OK;
}

extern "C" int hda_csr_download(hda_csr_t A, int *rowptr, int *col, double *val)
{
   HDA_TRY
   const DCsr &m = A->get();
   if (rowptr) m.rowptr.download(rowptr, (size_t)m.nrows + 1);
   if (col && m.nnz) m.col.download(col, (size_t)m.nnz);
   if (val && m.nnz) m.val.download(val, (size_t)m.nnz);
   HDA_CATCH
}

extern "C" int hda_lap7_create(const int n[3], const int P[3], const int pc[3], const double c[3],
                               hda_csr_t *A, double *rhs_host)
{
   HDA_TRY
   HDA_REQUIRE(P[0] == 1 && P[1] == 1 && P[2] == 1, "hda_lap7_create builds the single-block matrix; use the IJ path for partitions");
   const long long N = (long long)n[0] * n[1] * n[2];
   HDA_REQUIRE(N < (1LL << 31) / 7, "grid too large for int32 local indexing");
   auto h     = std::make_unique<hda_csr_s>();
   h->m.nrows = h->m.ncols = (int)N;
   h->m.rowptr.alloc((size_t)N + 1);
   const long long nnz = 7 * N - 2 * ((long long)n[0] * n[1] + (long long)n[1] * n[2] + (long long)n[0] * n[2]);
   h->m.nnz = (int)nnz;
   DArray<long long> cols64((size_t)nnz);
   h->m.col.alloc((size_t)nnz);
   h->m.val.alloc((size_t)nnz);
   h->rhs.alloc((size_t)N);
   lap7_generate(n, P, pc, c, h->m.rowptr.data(), cols64.data(), h->m.val.data(), h->rhs.data(), (int)N);
   k_cols64_to_32<<<2048, 256, 0, Context::get().stream>>>(nnz, cols64.data(), 0, h->m.col.data());
   sort_rows(h->m);
   if (rhs_host) h->rhs.download(rhs_host, (size_t)N);
   finish(h, A);
   HDA_CATCH
}

// ------------------------------------------------------------- K1 / K2 / K9

extern "C" int hda_spmv(hda_csr_t A, double alpha, const double *x, double beta, double *y)
{
   HDA_TRY
   const DCsr    &m  = A->get();
   DArray<double> dx = staged(x, m.ncols), dy = staged(y, m.nrows);
   spmv(m, alpha, dx.data(), beta, dy.data(), dy.data());
   fetch(dy.data(), y, m.nrows);
   HDA_CATCH
}

extern "C" int hda_relax(hda_csr_t A, int relax_type, double weight, int sweeps, const double *b, double *x)
{
   HDA_TRY
   const DCsr &m        = A->get();
   const bool  jacobi_t = is_jacobi_type(relax_type), gs_t = is_gs_type(relax_type), ts_t = is_two_stage_type(relax_type);
   HDA_REQUIRE(jacobi_t || gs_t || ts_t, "device relax: Jacobi (0/7/18), hybrid Gauss-Seidel (3/4/6/8/13/14) or two-stage Gauss-Seidel (11/12)");
   const bool     fwd = relax_type != 4 && relax_type != 14, bwd = relax_type != 3 && relax_type != 13; // the symmetric types sweep both ways
   DArray<double> dinv;
   build_dinv(m, relax_type, weight, dinv);
   const int      nx = std::max(m.ncols, m.nrows);
   DArray<double> db = staged(b, m.nrows), x0 = staged(x, m.nrows, nx), x1 = room<double>(nx);
   double *cur = x0.data(), *alt = x1.data();
   GsPlan  plan;
   if (gs_t) build_gs_plan(m, plan);
   TwoStage       ts;
   DArray<double> tz;
   if (ts_t)
   {
      two_stage_build(m, {}, ts);
      if (relax_type == 12) tz = room<double>(m.nrows);
   }
   for (int s = 0; s < sweeps; s++)
   {
      if (ts_t) two_stage_sweep(m, ts, dinv.data(), weight, db.data(), cur, alt, tz.data(), relax_type == 11 ? 1 : 2, false);
      else if (jacobi_t)
      {
         jacobi(m, dinv.data(), db.data(), cur, alt, -1);
         std::swap(cur, alt);
      }
      else
      {
         if (fwd) gs_sweep(m, plan, dinv.data(), db.data(), cur, true);
         if (bwd) gs_sweep(m, plan, dinv.data(), db.data(), cur, false);
      }
   }
   fetch(cur, x, m.nrows);
   gs_free_check(); // (an aborted barrier-free sweep is reported by the call that ran it, not by a later solve)
   HDA_CATCH
}

extern "C" int hda_relax_blocks(hda_csr_t A, int relax_type, double weight, int sweeps, int nblk, const int64_t *part, const double *b, double *x)
{
   HDA_TRY
   const DCsr &m    = A->get();
   const bool  gs_t = is_gs_type(relax_type), ts_t = is_two_stage_type(relax_type);
   HDA_REQUIRE(gs_t || ts_t, "row-block relax: hybrid Gauss-Seidel (3/4/6/8/13/14) or two-stage Gauss-Seidel (11/12)");
   const std::vector<int> hp = to_part(nblk, part, m.nrows);
   const int              nx = std::max(m.ncols, m.nrows);
   DArray<double>         dinv;
   if (ts_t)
   { // L restricted to every row's block; the divisors are the plain diagonal whatever the blocks
      TwoStage ts;
      two_stage_build(m, hp, ts);
      build_dinv(m, relax_type, weight, dinv);
      DArray<double> db = staged(b, m.nrows), x0 = staged(x, m.nrows, nx), r = room<double>(m.nrows), tz;
      if (relax_type == 12) tz = room<double>(m.nrows);
      for (int s = 0; s < sweeps; s++) two_stage_sweep(m, ts, dinv.data(), weight, db.data(), x0.data(), r.data(), tz.data(), relax_type == 11 ? 1 : 2, false);
      fetch(x0.data(), x, m.nrows);
      return HDA_OK;
   }
   GsPlan plan;
   build_gs_plan_blocks(m, hp, plan);
   build_dinv(m, relax_type, weight, dinv, plan.blk_part.data(), nblk);
   DArray<double> db = staged(b, m.nrows), x0 = staged(x, m.nrows, nx), x1 = room<double>(nx);
   double *cur = x0.data(), *alt = x1.data();
   const bool fwd = relax_type != 4 && relax_type != 14, bwd = relax_type != 3 && relax_type != 13; // the symmetric types sweep both ways
   for (int s = 0; s < sweeps; s++)
   {
      if (fwd)
      {
         gs_sweep_blocks(m, plan, dinv.data(), db.data(), cur, alt, true, false);
         std::swap(cur, alt);
      }
      if (bwd)
      {
         gs_sweep_blocks(m, plan, dinv.data(), db.data(), cur, alt, false, false);
         std::swap(cur, alt);
      }
   }
   fetch(cur, x, m.nrows);
   gs_free_check();
   HDA_CATCH
}

extern "C" int hda_l1_norms_blocks(hda_csr_t A, int option, int nblk, const int64_t *part, double *l1)
{
   HDA_TRY
   const DCsr            &m  = A->get();
   const std::vector<int> hp = to_part(nblk, part, m.nrows);
   DArray<int>            dp = staged(hp.data(), (int)hp.size());
   DArray<double>         d  = room<double>(m.nrows);
   l1_row_norms(m, option, d.data(), dp.data(), nblk);
   fetch(d.data(), l1, m.nrows);
   HDA_CATCH
}

extern "C" int hda_hmis_blocks(hda_csr_t A, const unsigned char *smask, int nblk, const int64_t *part, uint64_t seed, int level, int *cf)
{
   HDA_TRY
   const DCsr            &m  = A->get();
   const std::vector<int> hp = to_part(nblk, part, m.nrows);
   DArray<unsigned char>  sm  = staged(smask, m.nnz);
   DArray<int>            dcf = room<int>(m.nrows);
   amg_hmis(m, sm.data(), hp, seed, level, dcf.data());
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}

// CLJP / RS / Falgout coarsening; rounds (may be NULL): the CLJP rounds taken
extern "C" int hda_cljp(hda_csr_t A, const unsigned char *smask, uint64_t seed, int level, int64_t row_offset, int *cf, int *rounds)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = room<int>(m.nrows);
   const int             r   = amg_cljp(m, sm.data(), seed, level, row_offset, dcf.data());
   if (rounds) *rounds = r;
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}

extern "C" int hda_rs_blocks(hda_csr_t A, const unsigned char *smask, int nblk, const int64_t *part, int *cf)
{
   HDA_TRY
   const DCsr            &m  = A->get();
   const std::vector<int> hp = to_part(nblk, part, m.nrows);
   DArray<unsigned char>  sm  = staged(smask, m.nnz);
   DArray<int>            dcf = room<int>(m.nrows);
   amg_rs(m, sm.data(), hp, dcf.data());
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}

extern "C" int hda_falgout_blocks(hda_csr_t A, const unsigned char *smask, int nblk, const int64_t *part, uint64_t seed, int level, int *cf,
                                  int *rounds)
{
   HDA_TRY
   const DCsr            &m  = A->get();
   const std::vector<int> hp = to_part(nblk, part, m.nrows);
   DArray<unsigned char>  sm  = staged(smask, m.nnz);
   DArray<int>            dcf = room<int>(m.nrows);
   const int              r   = amg_falgout(m, sm.data(), hp, seed, level, dcf.data());
   if (rounds) *rounds = r;
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}

extern "C" int hda_measure_rnd(int n, uint64_t seed, int level, int64_t row_offset, double *rnd)
{
   HDA_TRY
   HDA_REQUIRE(n >= 0, "hda_measure_rnd: negative length");
   DArray<double> d = room<double>(n);
   amg_measure_rnd(n, seed, level, row_offset, d.data());
   fetch(d.data(), rnd, n);
   HDA_CATCH
}

extern "C" int hda_dot(int n, const double *x, const double *y, double *result)
{
   HDA_TRY
   DArray<double> dx = staged(x, n), dy = staged(y, n);
   dot(n, dx.data(), dy.data(), 0);
   finalize(0, S_TMP);
   *result = read_scalar(S_TMP);
   HDA_CATCH
}

extern "C" int hda_l1_norms(hda_csr_t A, int option, double *l1)
{
   HDA_TRY
   const DCsr    &m = A->get();
   DArray<double> d = room<double>(m.nrows);
   l1_row_norms(m, option, d.data());
   fetch(d.data(), l1, m.nrows);
   HDA_CATCH
}

// ------------------------------------------------------------- K4 / K5 / K6

extern "C" int hda_strength(hda_csr_t A, double theta, double max_row_sum, unsigned char *smask)
{
   HDA_TRY
   const DCsr           &m  = A->get();
   DArray<unsigned char> sm = room<unsigned char>(m.nnz);
   amg_strength(m, theta, max_row_sum, sm.data());
   fetch(sm.data(), smask, m.nnz);
   HDA_CATCH
}

extern "C" int hda_pmis(hda_csr_t A, const unsigned char *smask, uint64_t seed, int level,
                        int64_t row_offset, int *cf)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = room<int>(m.nrows);
   amg_pmis(m, sm.data(), seed, level, row_offset, dcf.data());
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}

// extended+i (6), direct (3), standard (8), mm-ext+i (17), extended (14), mm-ext (16) and one-point (100) interpolation for a given
// strength mask and splitting
static int interp_of_type(int interp_type, hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = staged(cf, m.nrows);
   auto                  h   = std::make_unique<hda_csr_s>();
   amg_interp_extpi(m, sm.data(), dcf.data(), pmax, trunc_factor, h->m, nullptr, interp_type);
   finish(h, P);
   HDA_CATCH
}
extern "C" int hda_interp_extpi(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(6, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_direct(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(3, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_standard(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(8, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_mm_extpi(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(17, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_extended(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(14, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_mm_ext(hda_csr_t A, const unsigned char *smask, const int *cf, int pmax, double trunc_factor, hda_csr_t *P)
{
   return interp_of_type(16, A, smask, cf, pmax, trunc_factor, P);
}
extern "C" int hda_interp_one_point(hda_csr_t A, const unsigned char *smask, const int *cf, hda_csr_t *P)
{
   return interp_of_type(100, A, smask, cf, 0, 0.0, P);
}

// aggressive coarsening pieces (hda_amg_agg.hip), one entry per stage for the per-kernel parity tests
extern "C" int hda_second_strength(hda_csr_t A, const unsigned char *smask, const int *cf, int num_paths, hda_csr_t *S2)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = staged(cf, m.nrows), c1;
   auto                  h   = std::make_unique<hda_csr_s>();
   amg_second_strength(m, sm.data(), dcf.data(), num_paths, h->m, c1);
   finish(h, S2);
   HDA_CATCH
}
extern "C" int hda_coarsen_second_pass(hda_csr_t A, const unsigned char *smask, int num_paths, uint64_t seed, int level, int *cf)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = staged(cf, m.nrows);
   amg_coarsen_second_pass(m, sm.data(), num_paths, seed, level, dcf.data());
   fetch(dcf.data(), cf, m.nrows);
   HDA_CATCH
}
extern "C" int hda_interp_multipass(hda_csr_t A, const unsigned char *smask, const int *cf, hda_csr_t *P)
{
   HDA_TRY
   const DCsr           &m   = A->get();
   DArray<unsigned char> sm  = staged(smask, m.nnz);
   DArray<int>           dcf = staged(cf, m.nrows);
   auto                  h   = std::make_unique<hda_csr_s>();
   amg_interp_multipass(m, sm.data(), dcf.data(), h->m);
   finish(h, P);
   HDA_CATCH
}

// two-stage mm-ext (plus_i 0) / mm-ext+i (1) interpolation of an aggressive level; P1 / P2 / P: the stages and the product (any may be NULL)
extern "C" int hda_interp_agg_two_stage(hda_csr_t A, const unsigned char *smask, const int *cf1, const int *cf2, int plus_i, int p12_pmax,
                                        double p12_trunc_factor, int pmax, double trunc_factor, hda_csr_t *P1, hda_csr_t *P2, hda_csr_t *P)
{
   HDA_TRY
   HDA_REQUIRE(A && smask && cf1 && cf2, "hda_interp_agg_two_stage: A, smask, cf1 and cf2 are required");
   const DCsr           &m  = A->get();
   DArray<unsigned char> sm = staged(smask, m.nnz);
   DArray<int>           d1 = staged(cf1, m.nrows), d2 = staged(cf2, m.nrows);
   auto h1 = std::make_unique<hda_csr_s>(), h2 = std::make_unique<hda_csr_s>(), h = std::make_unique<hda_csr_s>();
   if (!P1 && !P) amg_interp_mm_partial(m, sm.data(), d1.data(), d2.data(), pmax, trunc_factor, plus_i != 0, h2->m); // the second stage alone
   else amg_interp_agg_two_stage(m, sm.data(), d1.data(), d2.data(), plus_i != 0, p12_pmax, p12_trunc_factor, pmax, trunc_factor, h->m, &h1->m, &h2->m);
   Context::get().sync();
   if (P1) *P1 = h1.release();
   if (P2) *P2 = h2.release();
   if (P) *P = h.release();
   HDA_CATCH
}

extern "C" int hda_truncate_rows(hda_csr_t P, int pmax, double trunc_factor)
{
   HDA_TRY
   amg_truncate_rows(const_cast<DCsr &>(P->get()), pmax, trunc_factor);
   Context::get().sync();
   HDA_CATCH
}

extern "C" int hda_transpose(hda_csr_t A, hda_csr_t *T)
{
   HDA_TRY
   auto h = std::make_unique<hda_csr_s>();
   transpose(A->get(), h->m);
   finish(h, T);
   HDA_CATCH
}

extern "C" int hda_spgemm(hda_csr_t X, hda_csr_t Y, hda_csr_t *C)
{
   HDA_TRY
   auto h = std::make_unique<hda_csr_s>();
   spgemm(X->get(), Y->get(), h->m);
   finish(h, C);
   HDA_CATCH
}

extern "C" int hda_spgemm_last_route(int64_t out[8])
{
   HDA_TRY
   HDA_REQUIRE(out, "hda_spgemm_last_route: out is required");
   const SetupRoute &r = setup_route();
   out[0] = r.path; out[1] = r.why; out[2] = r.cap; out[3] = r.nt;
   out[4] = r.nchunks; out[5] = r.maxnp; out[6] = r.total; out[7] = r.batches;
   HDA_CATCH
}

extern "C" int hda_sort_rows_last_route(int64_t *route)
{
   HDA_TRY
   HDA_REQUIRE(route, "hda_sort_rows_last_route: route is required");
   *route = setup_route().sort;
   HDA_CATCH
}

extern "C" int hda_rap(hda_csr_t A, hda_csr_t P, hda_csr_t *Ac)
{
   HDA_TRY
   DCsr R;
   transpose(P->get(), R);
   auto h = std::make_unique<hda_csr_s>();
   amg_rap(A->get(), P->get(), R, h->m);
   finish(h, Ac);
   HDA_CATCH
}

extern "C" int hda_air_restriction(hda_csr_t A, const int *cf, int distance, double strong_th, double filter_th, hda_csr_t *R, int64_t stats[5])
{
   HDA_TRY
   HDA_REQUIRE(A && R && stats, "hda_air_restriction: A, R and stats are required");
   const DCsr &m = A->get();
   HDA_REQUIRE(m.nrows == m.ncols, "hda_air_restriction: the operator must be square");
   HDA_REQUIRE(cf || m.nrows == 0, "hda_air_restriction: cf is required");
   HDA_REQUIRE(distance == 1 || distance == 2, "hda_air_restriction: distance must be 1 (air_1) or 2 (air_2)");
   HDA_REQUIRE(std::isfinite(strong_th) && strong_th >= 0.0 && std::isfinite(filter_th) && filter_th >= 0.0,
               "hda_air_restriction: strong_th and filter_th must be finite and >= 0");
   DArray<int> dcf = staged(cf, m.nrows);
   auto        h   = std::make_unique<hda_csr_s>();
   long long   st[5];
   air_restriction(m, m.nrows ? dcf.data() : nullptr, distance, strong_th, filter_th, h->m, st);
   finish(h, R);
   for (int q = 0; q < 5; q++) stats[q] = st[q];
   HDA_CATCH
}

// ------------------------------------------------------------------ hierarchy

extern "C" int hda_amg_create_dof(const hda_amg_params *p, hda_csr_t A, const int *dof_func, hda_amg_t *out)
{
   HDA_TRY
   auto h = std::make_unique<hda_amg_s>();
   h->pc.owned_amg = std::make_unique<Amg>(to_params(p));
   h->pc.amg       = h->pc.owned_amg.get();
   h->pc.kind      = Precond::AMG;
   h->A            = A;
   if (dof_func) h->pc.amg->dof_func0.assign(dof_func, dof_func + A->get().nrows);
   h->pc.amg->setup(A->get());
   *out = h.release();
   HDA_CATCH
}
extern "C" int hda_amg_create(const hda_amg_params *p, hda_csr_t A, hda_amg_t *out) { return hda_amg_create_dof(p, A, nullptr, out); }
extern "C" int hda_amg_destroy(hda_amg_t h)
{
   if (!h) return HDA_OK;
   try { if (hda_device_count() > 0) Context::get().sync(); } catch (...) {}
   delete h;
   return HDA_OK;
}
extern "C" int hda_amg_num_levels(hda_amg_t h) { return (h && h->pc.amg) ? h->pc.amg->num_levels() : 0; }

// "preconditioner: ilu" (reference src/internal/ilu.c): a handle the Krylov entry points accept in place of a hierarchy
// on V row blocks (IluParams::blocks: bj-iluk at np = V; block_part = V + 1 row starts or NULL for hypre's even split)
extern "C" int hda_ilu_create_blocks(hda_csr_t A, int max_iter, int tri_solve, int lower_it, int upper_it, int blocks, const int64_t *block_part,
                                     hda_amg_t *out)
{
   HDA_TRY
   auto h = std::make_unique<hda_amg_s>();
   h->A       = A;
   h->pc.kind = Precond::ILU;
   h->pc.ilu  = std::make_unique<Ilu>();
   IluParams p;
   p.max_iter = max_iter; p.tri_solve = tri_solve; p.lower_it = lower_it; p.upper_it = upper_it;
   p.blocks   = blocks;
   if (block_part && blocks > 1) p.block_part.assign(block_part, block_part + blocks + 1);
   h->pc.ilu->setup(A->get(), p);
   *out = h.release();
   HDA_CATCH
}
extern "C" int hda_ilu_create(hda_csr_t A, int max_iter, int tri_solve, int lower_it, int upper_it, hda_amg_t *out)
{ // one block
   return hda_ilu_create_blocks(A, max_iter, tri_solve, lower_it, upper_it, 1, nullptr, out);
}
extern "C" int hda_ilu_blocks(hda_amg_t h, int level)
{
   if (!h) return 0;
   if (level < 0) return h->pc.ilu ? h->pc.ilu->blocks_used() : 0;
   if (!h->pc.amg || level >= h->pc.amg->num_levels() || !h->pc.amg->level(level).ilu) return 0;
   return h->pc.amg->level(level).ilu->blocks_used();
}
// "preconditioner: schwarz" (reference src/internal/schwarz.c): RAS / AS with ILU(k) subdomain solves (hda_schwarz.hip)
extern "C" int hda_schwarz_create(hda_csr_t A, int variant, int overlap, int fill, int blocks, const int64_t *block_part, int max_iter,
                                  double weight, hda_amg_t *out)
{
   HDA_TRY
   HDA_REQUIRE(A && out, "hda_schwarz_create: null argument");
   auto h     = std::make_unique<hda_amg_s>();
   h->A       = A;
   h->pc.kind    = Precond::SCHWARZ;
   h->pc.schwarz = std::make_unique<Schwarz>();
   SchwarzParams p;
   p.variant = variant; p.overlap = overlap; p.fill = fill; p.max_iter = max_iter; p.weight = weight;
   p.blocks  = blocks;
   if (block_part && blocks > 1) p.block_part.assign(block_part, block_part + blocks + 1);
   h->pc.schwarz->setup(A->get(), p);
   *out = h.release();
   HDA_CATCH
}
extern "C" int hda_schwarz_domains(hda_amg_t h, int *V, int *dom_ptr, int *dom_rows)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.schwarz, "not a Schwarz handle");
   const Schwarz &S = *h->pc.schwarz;
   if (V) *V = S.num_domains();
   if (dom_ptr)
   {
      const std::vector<int> v = S.dom_ptr_host();
      std::copy(v.begin(), v.end(), dom_ptr);
   }
   if (dom_rows && S.n_ext)
   {
      const std::vector<int> v = S.dom_rows_host();
      std::copy(v.begin(), v.begin() + S.n_ext, dom_rows);
   }
   HDA_CATCH
}
extern "C" int hda_schwarz_info(hda_amg_t h, int64_t info[6], double setup_ms[4])
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.schwarz && info, "not a Schwarz handle");
   const Schwarz &S = *h->pc.schwarz;
   info[0] = S.n_ext; info[1] = S.factors().nnz; info[2] = S.longest_row; info[3] = S.global_rows; info[4] = kSchwarzLdsRows; info[5] = S.nnz_A;
   if (setup_ms)
      for (int q = 0; q < 4; q++) setup_ms[q] = S.setup_ms[q];
   HDA_CATCH
}
// "preconditioner: fsai" (reference src/internal/fsai.c, algo_type bj-sfsai): the static FSAI of hda_fsai.hip
extern "C" int hda_fsai_create(hda_csr_t A, int num_levels, double threshold, int max_nnz_row, int eig_max_iters, int max_iter, int blocks,
                               const int64_t *block_part, hda_amg_t *out)
{
   HDA_TRY
   HDA_REQUIRE(A && out, "hda_fsai_create: null argument");
   auto h  = std::make_unique<hda_amg_s>();
   h->A       = A;
   h->pc.kind = Precond::FSAI;
   h->pc.fsai = std::make_unique<Fsai>();
   FsaiParams p;
   p.num_levels = num_levels; p.threshold = threshold; p.max_nnz_row = max_nnz_row; p.eig_max_iters = eig_max_iters; p.max_iter = max_iter;
   p.blocks = blocks;
   if (block_part && blocks > 1) p.block_part.assign(block_part, block_part + blocks + 1);
   h->pc.fsai->setup(A->get(), p);
   *out = h.release();
   HDA_CATCH
}
static Fsai *fsai_of(hda_amg_t h, int level)
{
   HDA_REQUIRE(h, "null handle");
   if (level < 0) return h->pc.fsai.get();
   HDA_REQUIRE(h->pc.amg && level < h->pc.amg->num_levels(), "level out of range");
   return h->pc.amg->level(level).fsai.get();
}
extern "C" int hda_fsai_factor(hda_amg_t h, int level, hda_csr_t *out)
{
   HDA_TRY
   const Fsai *F = fsai_of(h, level);
   HDA_REQUIRE(F && out, "no FSAI factor on this handle / level");
   lend(h, &F->factor(), out);
   HDA_CATCH
}
extern "C" int hda_fsai_info(hda_amg_t h, int level, int64_t info[9], double vals[6])
{
   HDA_TRY
   const Fsai *F = fsai_of(h, level);
   HDA_REQUIRE(F && info, "no FSAI factor on this handle / level");
   info[0] = F->n; info[1] = F->factor().nnz; info[2] = F->fallback_rows; info[3] = F->nblocks;
   for (int q = 0; q < 5; q++) info[4 + q] = F->class_rows[q];
   if (vals)
   {
      vals[0] = F->omega;
      vals[1] = F->apply_bytes();
      for (int q = 0; q < 4; q++) vals[2 + q] = F->setup_ms[q];
   }
   HDA_CATCH
}
// "preconditioner: ams" (reference src/internal/ams.c): auxiliary-space Maxwell preconditioner (hda_ams.hip)
extern "C" void hda_ams_default_amg_params(hda_amg_params *p, int num_functions)
{
   AmsAmgOptions o;
   o.agg_levels = 0; // (the reference's own default, 1, is refused for alpha: see ams_refusal)
   from_params(ams_subspace_amg(o, num_functions), p);
}
extern "C" int hda_ams_create(hda_csr_t A, hda_csr_t G, const double *c0, const double *c1, const double *c2, int dimension, int cycle_type,
                              int relax_times, double relax_weight, int max_iter, const hda_amg_params *alpha, const hda_amg_params *beta,
                              hda_amg_t *out)
{
   HDA_TRY
   HDA_REQUIRE(A && G && out && c0 && c1, "hda_ams_create: null argument");
   HDA_REQUIRE(dimension == 2 || c2, "hda_ams_create: the third coordinate vector is required in three dimensions");
   hda_amg_params da, db;
   hda_ams_default_amg_params(&da, dimension);
   hda_ams_default_amg_params(&db, 1);
   AmsParams p;
   p.dimension = dimension; p.cycle_type = cycle_type; p.relax_times = relax_times; p.relax_weight = relax_weight; p.max_iter = max_iter;
   p.alpha = to_params(alpha ? alpha : &da);
   p.beta  = to_params(beta ? beta : &db);
   const DCsr    &g = G->get();
   DArray<double> c[3];
   const double  *hc[3] = {c0, c1, c2}, *dc[3] = {nullptr, nullptr, nullptr};
   for (int k = 0; k < dimension && k < 3; k++)
   {
      c[k]  = staged(hc[k], g.ncols);
      dc[k] = c[k].data();
   }
   auto h = std::make_unique<hda_amg_s>();
   h->A       = A;
   h->pc.kind = Precond::AMS;
   h->pc.ams  = std::make_unique<Ams>();
   h->pc.ams->setup(A->get(), g, dc, p);
   *out = h.release();
   HDA_CATCH
}
extern "C" int hda_ams_matrix(hda_amg_t h, int which, hda_csr_t *out)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.ams && out, "not an AMS handle");
   HDA_REQUIRE(which >= 0 && which <= 2, "which: 0 Pi, 1 G^T A G, 2 Pi^T A Pi");
   lend(h, (which == 0) ? &h->pc.ams->pi() : (which == 1) ? &h->pc.ams->a_g() : &h->pc.ams->a_pi(), out);
   HDA_CATCH
}
extern "C" int hda_ams_info(hda_amg_t h, int64_t info[8], double ms[5])
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.ams && info, "not an AMS handle");
   Ams &S  = *h->pc.ams;
   info[0] = S.n_e; info[1] = S.n_v; info[2] = S.pi().nnz; info[3] = S.a_g().nnz; info[4] = S.a_pi().nnz;
   info[5] = S.fixed_rows[0]; info[6] = S.fixed_rows[1]; info[7] = 256 * S.b_g().num_levels() + S.b_pi().num_levels();
   if (ms)
   {
      for (int q = 0; q < 4; q++) ms[q] = S.setup_ms[q];
      ms[4] = S.apply_bytes();
   }
   HDA_CATCH
}
extern "C" int hda_precond_time(hda_amg_t h, int reps, double *avg_ms)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.kind != Precond::NONE && !h->pc.amg && avg_ms && reps > 0,
               "hda_precond_time: an ILU, Schwarz, AMS or FSAI handle and reps > 0 are needed");
   Context       &ctx = Context::get();
   const DCsr    &m   = h->A->get();
   const size_t   nv  = h->pc.vec_len(m);
   DArray<double> b(nv), x(nv);
   fill((int)nv, 0.5, b.data());
   auto launch = [&]() { h->pc.solve(m, nullptr, b.data(), x.data(), true); };
   for (int w = 0; w < 3; w++) launch();
   hipEvent_t e0, e1;
   HDA_HIP(hipEventCreate(&e0));
   HDA_HIP(hipEventCreate(&e1));
   HDA_HIP(hipEventRecord(e0, ctx.stream));
   for (int r = 0; r < reps; r++) launch();
   HDA_HIP(hipEventRecord(e1, ctx.stream));
   HDA_HIP(hipEventSynchronize(e1));
   float ms = 0.f;
   HDA_HIP(hipEventElapsedTime(&ms, e0, e1));
   HDA_HIP(hipEventDestroy(e0));
   HDA_HIP(hipEventDestroy(e1));
   *avg_ms = ms / reps;
   gs_free_check();
   HDA_CATCH
}
// "preconditioner: mgr" (reference src/internal/mgr.c): multigrid reduction by dof labels
extern "C" int hda_mgr_create(hda_csr_t A, const int *labels, int nlevels, const hda_mgr_level_params *levels,
                              const hda_amg_params *coarsest_amg, int max_iter, hda_amg_t *out)
{
   HDA_TRY
   HDA_REQUIRE(labels && levels && nlevels > 0, "hda_mgr_create: labels and at least one level are needed");
   MgrParams p;
   p.coarse   = to_params(coarsest_amg);
   p.max_iter = max_iter;
   if (!coarsest_amg)
   { // coarsest_level: ilu -- its arguments ride in the last level's entry
      const hda_mgr_level_params &q = levels[nlevels - 1];
      p.coarse_is_ilu        = true;
      p.coarse_ilu.max_iter  = q.coarse_ilu_max_iter; p.coarse_ilu.tri_solve = q.coarse_ilu_tri_solve;
      p.coarse_ilu.lower_it  = q.coarse_ilu_lower_it; p.coarse_ilu.upper_it = q.coarse_ilu_upper_it;
   }
   for (int l = 0; l < nlevels; l++)
   {
      MgrLevelParams q;
      q.f_labels.assign(levels[l].f_labels, levels[l].f_labels + levels[l].n_f_labels);
      q.interp_type = levels[l].interp_type; q.restrict_type = levels[l].restrict_type;
      q.frelax_type = levels[l].frelax_type; q.frelax_sweeps = levels[l].frelax_sweeps;
      q.grelax_type = levels[l].grelax_type; q.grelax_sweeps = levels[l].grelax_sweeps;
      q.grelax_blocks = levels[l].grelax_blocks;
      q.coarse_type = levels[l].coarse_type; q.nonglk_max_elmts = levels[l].nonglk_max_elmts; q.coarse_th = levels[l].coarse_th;
      if (levels[l].frelax_amg) q.frelax_amg = to_params(levels[l].frelax_amg);
      q.ilu.tri_solve = levels[l].ilu_tri_solve; q.ilu.lower_it = levels[l].ilu_lower_it; q.ilu.upper_it = levels[l].ilu_upper_it;
      auto nested = [](const hda_krylov_params &k) {
         NestedKrylov r;
         r.max_iter = k.max_iter; r.rtol = k.rtol; r.atol = k.atol; r.two_norm = k.two_norm; r.krylov_dim = k.krylov_dim;
         return r;
      };
      if (levels[l].frelax_krylov > 0)
      {
         q.fkrylov_method  = levels[l].frelax_krylov - 1;
         q.fkrylov         = nested(levels[l].frelax_kp);
         q.fkrylov_precond = levels[l].frelax_krylov_precond != 0;
      }
      if (l == nlevels - 1)
      {
         if (levels[l].mgr_cycle > 0) p.cycle = levels[l].mgr_cycle;
         if (levels[l].mgr_frelax_pos > 0) p.frelax_pos = levels[l].mgr_frelax_pos;
         if (levels[l].mgr_gsmooth_pos > 0) p.gsmooth_pos = levels[l].mgr_gsmooth_pos;
      }
      if (l == nlevels - 1 && levels[l].coarse_krylov > 0)
      {
         p.ckrylov_method  = levels[l].coarse_krylov - 1;
         p.ckrylov         = nested(levels[l].coarse_kp);
         p.ckrylov_precond = levels[l].coarse_krylov_precond != 0;
      }
      p.levels.push_back(q);
   }
   auto h = std::make_unique<hda_amg_s>();
   h->A   = A;
   p.keep_blocks = true; // (this handle serves the test entry hda_mgr_blk_inverses)
   h->pc.kind = Precond::MGR;
   h->pc.mgr  = std::make_unique<Mgr>(p);
   h->pc.mgr->setup(A->get(), std::vector<int>(labels, labels + A->get().nrows));
   *out = h.release();
   HDA_CATCH
}
// borrowed view: which 0 operator of the level (level == reduction levels: the coarsest system), 1 P, 2 R
extern "C" int hda_mgr_matrix(hda_amg_t h, int level, int which, hda_csr_t *out)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.mgr, "not an MGR handle");
   lend(h, &h->pc.mgr->matrix(level, which), out);
   HDA_CATCH
}
extern "C" int hda_mgr_blk_inverses(hda_amg_t h, int level, int tier, double *out, int *b, int *nf)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.mgr && b && nf, "not an MGR handle");
   const std::vector<double> v = h->pc.mgr->block_inverses(level, tier, *b, *nf);
   if (out && !v.empty()) std::copy(v.begin(), v.end(), out);
   HDA_CATCH
}
// host wall time of an MGR setup per reduction level, then of the coarsest solver (tools/mgr_blk_setup.py); *n in: capacity, out: count
extern "C" int hda_mgr_setup_ms(hda_amg_t h, double *out, int *n)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.mgr && n, "not an MGR handle");
   const std::vector<double> &v = h->pc.mgr->level_ms;
   if (out) std::copy(v.begin(), v.begin() + std::min<size_t>(v.size(), (size_t)std::max(*n, 0)), out);
   *n = (int)v.size();
   HDA_CATCH
}
// factors (strict lower part L with unit diagonal, rest U) of the stand-alone handle (level < 0) or of
// the complex smoother of an AMG level
extern "C" int hda_ilu_factors(hda_amg_t h, int level, hda_csr_t *out)
{
   HDA_TRY
   const Ilu *F = nullptr;
   if (level < 0 && h->pc.schwarz)
   { // the block-diagonal factors of all subdomains, extended numbering
      lend(h, &h->pc.schwarz->factors(), out);
      return HDA_OK;
   }
   if (level < 0) F = h->pc.ilu.get();
   else
   {
      HDA_REQUIRE(h->pc.amg && level < h->pc.amg->num_levels(), "level out of range");
      F = h->pc.amg->level(level).ilu.get();
   }
   HDA_REQUIRE(F, "no ILU factorisation on this handle / level");
   lend(h, &F->factors(), out);
   HDA_CATCH
}

extern "C" int hda_amg_level_matrix(hda_amg_t h, int level, int which, hda_csr_t *out)
{
   HDA_TRY
   HDA_REQUIRE(level >= 0 && level < h->pc.amg->num_levels(), "level out of range");
   const DCsr *m = nullptr;
   if (which == 0) m = &h->pc.amg->level_A(level);
   else
   {
      HDA_REQUIRE(level < h->pc.amg->num_levels() - 1, "no transfer operator on the coarsest level");
      HDA_REQUIRE(which >= 1 && which <= 3, "which: 0 operator, 1 P, 2 R, 3 the folded up-leg operator");
      HDA_REQUIRE(which != 3 || h->pc.amg->level_folded(level), "the up leg of this level is not folded");
      m = (which == 1) ? &h->pc.amg->level(level).P : (which == 2) ? &h->pc.amg->level(level).R : &h->pc.amg->level(level).Pt;
   }
   lend(h, m, out);
   HDA_CATCH
}
extern "C" int hda_amg_fold_sweep(hda_amg_t h, int level, const double *dinv, const double *t, const double *e, const double *u, double *out)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.amg && dinv && t && e && u && out, "hda_amg_fold_sweep: null argument");
   HDA_REQUIRE(h->pc.amg->level_folded(level), "the up leg of this level is not folded");
   const DCsr    &A  = h->pc.amg->level_A(level), &M = h->pc.amg->level(level).Pt;
   DArray<double> dd = staged(dinv, M.nrows), dt = staged(t, M.nrows), de = staged(e, M.ncols), du = staged(u, M.nrows);
   DArray<double> dout = staged(out, M.nrows); // rows the sweep leaves alone come back as they were given
   jacobi_folded(A, M, dd.data(), dt.data(), de.data(), du.data(), dout.data());
   fetch(dout.data(), out, M.nrows);
   HDA_CATCH
}
// one level-0 Jacobi sweep as the cycle launches it (Amg::level0_sweep); *dot (may be null): <b, out> from the sweep's fused partials;
// *by_class: whether the divisors came from the row-class table
extern "C" int hda_amg_level0_sweep(hda_amg_t h, int dir, const double *b, const double *x, double *out, double *dot, int *by_class)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.amg && b && x && out && by_class, "hda_amg_level0_sweep: null argument");
   const DCsr    &A = h->pc.amg->level_A(0);
   DArray<double> db = staged(b, A.nrows), dx = staged(x, A.nrows, A.ncols), dout = room<double>(A.nrows);
   *by_class = h->pc.amg->level0_sweep(dir, db.data(), dx.data(), dout.data(), dot ? 0 : -1) ? 1 : 0;
   if (dot)
   {
      finalize(0, S_TMP);
      *dot = read_scalar(S_TMP);
   }
   fetch(dout.data(), out, A.nrows);
   HDA_CATCH
}
// the hierarchy's level 0 on another matrix of the same size, divisors and coarse levels kept (Amg::rebind: preconditioner reuse)
extern "C" int hda_amg_rebind(hda_amg_t h, hda_csr_t A)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.amg && A, "hda_amg_rebind: null argument");
   h->pc.amg->rebind(A->get(), nullptr);
   HDA_CATCH
}
extern "C" int hda_amg_level_cf(hda_amg_t h, int level, int *cf)
{
   HDA_TRY
   HDA_REQUIRE(level >= 0 && level < h->pc.amg->num_levels() - 1, "level has no C/F splitting");
   auto &L = h->pc.amg->level(level);
   L.cf.download(cf, L.cf.size());
   HDA_CATCH
}
extern "C" int hda_amg_blocks(hda_amg_t h) { return (h && h->pc.amg) ? h->pc.amg->blocks_used : 0; }
extern "C" int hda_amg_level_blocks(hda_amg_t h, int level, int64_t *part)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.amg && level >= 0 && level < h->pc.amg->num_levels(), "no such level");
   const std::vector<int> &bp = h->pc.amg->level_blocks(level);
   if (bp.size() < 2) { part[0] = 0; part[1] = h->pc.amg->level_A(level).nrows; }
   else for (size_t q = 0; q < bp.size(); q++) part[q] = bp[q];
   HDA_CATCH
}
extern "C" int hda_amg_complexities(hda_amg_t h, double *grid, double *op)
{
   if (!h) return HDA_ERR_ARG;
   if (grid) *grid = h->pc.amg->grid_complexity();
   if (op) *op = h->pc.amg->operator_complexity();
   return HDA_OK;
}
extern "C" double hda_amg_vcycle_bytes(hda_amg_t h) { return h ? h->pc.amg->vcycle_bytes() : 0.0; }

extern "C" int hda_amg_vcycle(hda_amg_t h, const double *b, double *x)
{ // one application of the preconditioner from a zero guess
   HDA_TRY
   const DCsr    &m = h->pc.amg ? h->pc.amg->level_A(0) : h->A->get();
   DArray<double> db = staged(b, m.nrows), dx = room<double>(std::max((int)h->pc.vec_len(m), m.ncols));
   h->pc.solve(m, nullptr, db.data(), dx.data(), true);
   fetch(dx.data(), x, m.nrows);
   gs_free_check();
   HDA_CATCH
}

// --------------------------------------------------------------------- Krylov

static int run_krylov(int kind, hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, const double *b,
                      double *x, double *hist, int *iters, int *converged, double *final_rel)
{
   HDA_TRY
   const DCsr    &m = A->get();
   DArray<double> db = staged(b, m.nrows), dx = staged(x, m.nrows, m.ncols);
   PrecondFn      M;
   if (amg) M = amg->pc.as_fn(m, nullptr);
   KrylovParams  k   = to_kparams(kp);
   LinOp         op(m, nullptr, (amg && amg->pc.amg) ? amg->pc.amg->vec_len0() : 0);
   KrylovResult  res = kind == 1 ? gmres(op, M, k, db.data(), dx.data()) : kind == 2 ? fgmres(op, M, k, db.data(), dx.data())
                     : kind == 3 ? bicgstab(op, M, k, db.data(), dx.data()) : pcg(op, M, k, db.data(), dx.data());
   fetch(dx.data(), x, m.nrows);
   if (hist)
      for (size_t i = 0; i < res.hist.size() && i < (size_t)k.max_iter + 1; i++) hist[i] = res.hist[i];
   if (iters) *iters = res.iters;
   if (converged) *converged = res.converged ? 1 : 0;
   if (final_rel) *final_rel = res.final_rel;
   HDA_CATCH
}
extern "C" int hda_pcg(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, const double *b, double *x,
                       double *hist, int *iters, int *converged, double *final_rel)
{
   return run_krylov(0, A, amg, kp, b, x, hist, iters, converged, final_rel);
}
extern "C" int hda_gmres(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, const double *b, double *x,
                         double *hist, int *iters, int *converged, double *final_rel)
{
   return run_krylov(1, A, amg, kp, b, x, hist, iters, converged, final_rel);
}
extern "C" int hda_fgmres(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, const double *b, double *x,
                          double *hist, int *iters, int *converged, double *final_rel)
{
   return run_krylov(2, A, amg, kp, b, x, hist, iters, converged, final_rel);
}
extern "C" int hda_bicgstab(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, const double *b, double *x,
                            double *hist, int *iters, int *converged, double *final_rel)
{
   return run_krylov(3, A, amg, kp, b, x, hist, iters, converged, final_rel);
}

// ------------------------------------------------- up to 8 right-hand sides at once

static int multi_width_checked(int k)
{
   const std::string why = multi_refusal(k);
   if (!why.empty()) throw Error(why);
   return multi_width(k);
}
// k host vectors of n (vector j at host + j * n; k * n values are read) interleaved over K columns: max(n, 1) * K elements, padding zero
static DArray<double> staged_multi(const double *host, int k, int n, int K)
{
   DArray<double> cm = staged(host, k * n), d((size_t)std::max(n, 1) * K);
   if (n == 0) d.zero();
   multi_pack(n, k, K, cm.data(), n, d.data());
   return d;
}
// ... and the k columns of n x K interleaved results back: exactly k * n values
static void fetch_multi(const double *dev, double *host, int k, int n, int K)
{
   DArray<double> cm = room<double>(k * n);
   multi_unpack(n, k, K, dev, cm.data(), n);
   fetch(cm.data(), host, k * n);
}
// the first k entries of a scalar block
static void fetch_block(int block, double *host, int k)
{
   fetch(MultiScratch::get().block(block), host, k);
}

extern "C" int hda_spmm(hda_csr_t A, int mode, int k, double alpha, double beta, const double *X, const double *Yin, const double *B, const double *dinv,
                        const double *W, double *Y, double *dots)
{
   HDA_TRY
   const DCsr &m = A->get();
   const int   K = multi_width_checked(k);
   HDA_REQUIRE(X && Y, "hda_spmm: X and Y are required");
   HDA_REQUIRE(mode == HDA_SPMM_PLAIN || mode == HDA_SPMM_RESID || mode == HDA_SPMM_JACOBI, "hda_spmm: unknown mode");
   HDA_REQUIRE(mode != HDA_SPMM_PLAIN || beta == 0.0 || Yin, "hda_spmm: beta != 0 needs Yin");
   HDA_REQUIRE(mode == HDA_SPMM_PLAIN || B, "hda_spmm: the residual and the Jacobi sweep need B");
   HDA_REQUIRE(mode != HDA_SPMM_JACOBI || (dinv && m.nrows <= m.ncols), "hda_spmm: the Jacobi sweep needs dinv and reads x[i] of every row (ncols >= nrows)");
   HDA_REQUIRE(!W || dots, "hda_spmm: W needs dots");
   // X: k x ncols; Yin, B, W, Y: k x nrows; dinv: nrows
   DArray<double> dX = staged_multi(X, k, m.ncols, K), dY = staged_multi(Y, k, m.nrows, K), dYin, dB, dW, dd;
   if (Yin && mode == HDA_SPMM_PLAIN) dYin = staged_multi(Yin, k, m.nrows, K);
   if (B && mode != HDA_SPMM_PLAIN) dB = staged_multi(B, k, m.nrows, K);
   if (W) dW = staged_multi(W, k, m.nrows, K);
   if (mode == HDA_SPMM_JACOBI) dd = staged(dinv, m.nrows);
   spmm(m, K, mode, alpha, dX.data(), beta, dYin.data(), dB.data(), dd.data(), W ? dW.data() : nullptr, dY.data(), W ? MS_TMP : -1);
   if (W)
   {
      if (m.nrows > 0)
      {
         multi_finalize(K, MS_TMP, 1, MV_TMP);
         fetch_block(MV_TMP, dots, k);
      }
      else
         for (int j = 0; j < k; j++) dots[j] = 0.0;
   }
   fetch_multi(dY.data(), Y, k, m.nrows, K);
   HDA_CATCH
}

extern "C" int hda_multi_blas(int op, int k, int n, const double *alpha, const double *beta, const int *active, const double *P, const double *S,
                              double *U, double *V, double *out)
{
   HDA_TRY
   const int K = multi_width_checked(k);
   HDA_REQUIRE(n >= 0 && U, "hda_multi_blas: n >= 0 and U are required");
   // alpha, beta, active, out: k entries; P, S, U, V: k x n
   int flags[kMultiMax];
   for (int j = 0; j < kMultiMax; j++) flags[j] = j < k && (!active || active[j]);
   multi_set_active(flags);
   DArray<double> dU = staged_multi(U, k, n, K);
   if (op == HDA_MBLAS_DOT)
   {
      HDA_REQUIRE(V && out, "hda_multi_blas: the dot products need V and out");
      DArray<double> dV = staged_multi(V, k, n, K);
      multi_dot(n, K, dU.data(), dV.data(), MS_TMP);
      multi_finalize(K, MS_TMP, 1, MV_TMP);
      fetch_block(MV_TMP, out, k);
   }
   else if (op == HDA_MBLAS_UPDATE)
   {
      HDA_REQUIRE(alpha && P && S && V && out, "hda_multi_blas: the update needs alpha, P, S, V and out");
      DArray<double> dV = staged_multi(V, k, n, K), dP = staged_multi(P, k, n, K), dS = staged_multi(S, k, n, K), da = staged(alpha, k, kMultiMax);
      multi_masked(K, da.data(), MV_ALPHA);
      multi_cg_update(n, K, MultiScratch::get().block(MV_ALPHA), dP.data(), dS.data(), dU.data(), dV.data(), MS_RR);
      multi_finalize(K, MS_RR, 1, MV_TMP);
      fetch_block(MV_TMP, out, k);
      fetch_multi(dU.data(), U, k, n, K);
      fetch_multi(dV.data(), V, k, n, K);
   }
   else if (op == HDA_MBLAS_DIR)
   {
      HDA_REQUIRE(beta && P, "hda_multi_blas: the direction step needs beta and P");
      DArray<double> dP = staged_multi(P, k, n, K), db = staged(beta, k, kMultiMax);
      multi_masked(K, db.data(), MV_BETA);
      multi_cg_dir(n, K, MultiScratch::get().block(MV_BETA), dP.data(), dU.data());
      fetch_multi(dU.data(), U, k, n, K);
   }
   else throw Error("hda_multi_blas: unknown op");
   HDA_CATCH
}

extern "C" int hda_amg_vcycle_multi(hda_amg_t h, int k, const double *B, double *X)
{
   HDA_TRY
   HDA_REQUIRE(h && h->pc.amg, "hda_amg_vcycle_multi: the handle is not a BoomerAMG hierarchy");
   HDA_REQUIRE(B && X, "hda_amg_vcycle_multi: B and X are required");
   const int      K = multi_width_checked(k);
   const DCsr    &m = h->pc.amg->level_A(0);
   DArray<double> dB = staged_multi(B, k, m.nrows, K), dX = room<double>(std::max(m.nrows, 1) * K); // B, X: k x n
   h->pc.amg->apply_multi(dB.data(), dX.data(), K);
   fetch_multi(dX.data(), X, k, m.nrows, K);
   HDA_CATCH
}

extern "C" int hda_pcg_multi(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, int k, const double *B, double *X, double *hist, int *iters,
                             int *converged, double *final_rel)
{
   HDA_TRY
   const DCsr &m = A->get();
   const int   K = multi_width_checked(k);
   HDA_REQUIRE(B && X, "hda_pcg_multi: B and X are required");
   HDA_REQUIRE(!amg || amg->pc.amg, "hda_pcg_multi: the preconditioner must be a BoomerAMG hierarchy or NULL");
   KrylovParams   kk = to_kparams(kp);
   DArray<double> dB = staged_multi(B, k, m.nrows, K), dX = staged_multi(X, k, m.nrows, K); // B, X: k x n
   const std::vector<KrylovResult> res = pcg_multi(m, amg ? amg->pc.amg : nullptr, kk, k, dB.data(), dX.data());
   fetch_multi(dX.data(), X, k, m.nrows, K);
   for (int j = 0; j < k; j++)
   { // hist: k x (max_iter + 1); iters, converged, final_rel: k
      const KrylovResult &r = res[(size_t)j];
      if (hist)
         for (size_t i = 0; i < r.hist.size() && i < (size_t)kk.max_iter + 1; i++) hist[(size_t)j * ((size_t)kk.max_iter + 1) + i] = r.hist[i];
      if (iters) iters[j] = r.iters;
      if (converged) converged[j] = r.converged ? 1 : 0;
      if (final_rel) final_rel[j] = r.final_rel;
   }
   HDA_CATCH
}

extern "C" int hda_time_kernel_multi(int kind, hda_csr_t A, hda_amg_t amg, int k, int reps, double *avg_ms, double *bytes)
{
   HDA_TRY
   Context       &ctx = Context::get();
   const DCsr    &m   = A->get();
   const int      K   = multi_width_checked(k);
   const size_t   nv  = (size_t)std::max(std::max(m.ncols, m.nrows), 1);
   DArray<double> x(nv * K), y(nv * K), b(nv * K), dinv(nv);
   fill((int)(nv * K), 1.0, x.data());
   fill((int)(nv * K), 0.5, b.data());
   {
      DArray<double> d((size_t)std::max(m.nrows, 1));
      l1_row_norms(m, 1, d.data());
      make_dinv(m.nrows, d.data(), 1.0, dinv.data());
   }
   HDA_REQUIRE(kind != 3 || (amg && amg->pc.amg), "batched V-cycle timing needs a hierarchy");
   auto launch = [&]() {
      switch (kind)
      {
         case 0: spmm(m, K, MM_PLAIN, 1.0, x.data(), 0.0, nullptr, nullptr, nullptr, nullptr, y.data(), -1); break;
         case 1: spmm(m, K, MM_JACOBI, 1.0, x.data(), 0.0, nullptr, b.data(), dinv.data(), nullptr, y.data(), -1); break;
         case 2: spmm(m, K, MM_RESID, 1.0, x.data(), 0.0, nullptr, b.data(), nullptr, nullptr, y.data(), -1); break;
         case 3: amg->pc.amg->apply_multi(b.data(), y.data(), K); break;
         default: throw Error("unknown kernel kind");
      }
   };
   for (int w = 0; w < 3; w++) launch();
   hipEvent_t e0, e1;
   HDA_HIP(hipEventCreate(&e0));
   HDA_HIP(hipEventCreate(&e1));
   HDA_HIP(hipEventRecord(e0, ctx.stream));
   for (int r = 0; r < reps; r++) launch();
   HDA_HIP(hipEventRecord(e1, ctx.stream));
   HDA_HIP(hipEventSynchronize(e1));
   float ms = 0.f;
   HDA_HIP(hipEventElapsedTime(&ms, e0, e1));
   (void)hipEventDestroy(e0);
   (void)hipEventDestroy(e1);
   if (avg_ms) *avg_ms = (double)ms / std::max(reps, 1);
   if (bytes) *bytes = kind == 3 ? amg->pc.amg->vcycle_multi_bytes(K) : spmm_bytes(m, K, kind == 0 ? MM_PLAIN : kind == 1 ? MM_JACOBI : MM_RESID, false);
   HDA_CATCH
}

// ---------------------------------------------------------------- measurement

static double spmv_alg_bytes(const DCsr &M) { return 12.0 * M.nnz + 4.0 * (M.nrows + 1.0) + 8.0 * M.ncols + 8.0 * M.nrows; }

extern "C" int hda_time_kernel(int kind, hda_csr_t A, hda_amg_t amg, int reps, double *avg_ms, double *bytes)
{
   HDA_TRY
   Context       &ctx = Context::get();
   const DCsr    &m   = A->get();
   const size_t   nv  = (size_t)std::max(std::max(m.ncols, m.nrows), 1); // x needs ncols, y/b/dinv need nrows
   DArray<double> x(nv), y(nv), b(nv), dinv(nv);
   fill((int)nv, 1.0, x.data());
   fill((int)nv, 0.5, b.data());
   {
      DArray<double> d((size_t)m.nrows);
      l1_row_norms(m, 1, d.data());
      make_dinv(m.nrows, d.data(), 1.0, dinv.data());
   }
   auto launch = [&]() {
      switch (kind)
      {
         case 0: spmv(m, 1.0, x.data(), 0.0, nullptr, y.data()); break;
         case 1: jacobi(m, dinv.data(), b.data(), x.data(), y.data(), -1); break;
         case 2: residual(m, x.data(), b.data(), y.data()); break;
         case 3:
            HDA_REQUIRE(amg, "V-cycle timing needs a hierarchy");
            HDA_REQUIRE(nv >= amg->pc.amg->vec_len0(), "vector too short for the hierarchy");
            amg->pc.amg->apply(b.data(), y.data(), -1);
            break;
         default: throw Error("unknown kernel kind");
      }
   };
   for (int w = 0; w < 3; w++) launch();
   hipEvent_t e0, e1;
   HDA_HIP(hipEventCreate(&e0));
   HDA_HIP(hipEventCreate(&e1));
   HDA_HIP(hipEventRecord(e0, ctx.stream));
   for (int r = 0; r < reps; r++) launch();
   HDA_HIP(hipEventRecord(e1, ctx.stream));
   HDA_HIP(hipEventSynchronize(e1));
   float ms = 0.f;
   HDA_HIP(hipEventElapsedTime(&ms, e0, e1));
   (void)hipEventDestroy(e0);
   (void)hipEventDestroy(e1);
   if (avg_ms) *avg_ms = (double)ms / std::max(reps, 1);
   if (bytes)
   {
      const double sb = spmv_alg_bytes(m);
      *bytes = (kind == 0) ? sb : (kind == 1) ? sb + 16.0 * m.nrows : (kind == 2) ? sb + 8.0 * m.nrows : amg->pc.amg->vcycle_bytes();
   }
   HDA_CATCH
}

extern "C" void hda_set_overlap(int mode) { set_overlap_mode(mode); }
extern "C" int hda_last_precond_calls(void) { return last_precond_calls(); }

extern "C" int hda_solve_device(hda_csr_t A, hda_amg_t amg, const hda_krylov_params *kp, int solver,
                                const double *b_host, int nsolves, double *solve_ms, int *iters,
                                double *final_rel, double *r0_norm, double *true_rel, double *k1_avg_ms)
{
   HDA_TRY
   using clk        = std::chrono::steady_clock;
   Context       &ctx = Context::get();
   const DCsr    &m   = A->get();
   const int      n   = m.nrows;
   DArray<double> b, x(std::max<size_t>((size_t)std::max(m.ncols, 1), amg && amg->pc.amg ? amg->pc.amg->vec_len0() : 0)), r((size_t)std::max(n, 1));
   if (b_host) b.upload(b_host, (size_t)n);
   else if (A->rhs_ref)
   {
      b.alloc((size_t)std::max(n, 1));
      copy(n, A->rhs_ref, b.data());
   }
   else
   {
      HDA_REQUIRE(A->rhs.size() == (size_t)n, "no right-hand side: pass b or build A with hda_lap7_create");
      b.copy_from(A->rhs);
   }
   x.zero();
   const bool multi = A->halo && Comm::world().size > 1;
   // initial residual norm, untimed (solver.c:666)
   residual(m, x.data(), b.data(), r.data()); // x = 0: no ghost refresh needed
   dot(n, r.data(), r.data(), 0);
   finalize(0, S_TMP);
   const double r0 = std::sqrt(read_scalar(S_TMP));
   dot(n, b.data(), b.data(), 0);
   finalize(0, S_TMP);
   const double bn = std::sqrt(read_scalar(S_TMP));
   PrecondFn M;
   if (amg) M = [amg](const double *rr, double *zz, int slot) { amg->pc.amg->apply_offering(rr, zz, slot); };
   KrylovParams k = to_kparams(kp);
   k.profile_k1   = (k1_avg_ms != nullptr);
   LinOp op(m, multi ? A->halo : nullptr, amg ? amg->pc.amg->vec_len0() : 0);
   KrylovResult res;
   double       k1_sum = 0.0;
   long         k1_cnt = 0;
   for (int s = 0; s < std::max(nsolves, 1); s++)
   {
      x.zero(); // HYPREDRV_LinearSystemResetInitialGuess
      ctx.sync();
      auto t0 = clk::now();
      res     = solver ? gmres(op, M, k, b.data(), x.data()) : pcg(op, M, k, b.data(), x.data());
      ctx.sync();
      auto t1 = clk::now();
      if (solve_ms) solve_ms[s] = std::chrono::duration<double, std::milli>(t1 - t0).count();
      k1_sum += res.k1_ms_sum;
      k1_cnt += res.k1_count;
   }
   // true relative residual, untimed (solver.c:686-690)
   if (multi) halo_exchange(*A->halo, x.data());
   residual(m, x.data(), b.data(), r.data());
   dot(n, r.data(), r.data(), 0);
   finalize(0, S_TMP);
   const double rn = std::sqrt(read_scalar(S_TMP));
   if (iters) *iters = res.iters;
   if (final_rel) *final_rel = res.final_rel;
   if (r0_norm) *r0_norm = r0;
   if (true_rel) *true_rel = (bn > 0.0) ? rn / bn : rn;
   if (k1_avg_ms) *k1_avg_ms = k1_cnt ? k1_sum / (double)k1_cnt : 0.0;
   HDA_CATCH
}

extern "C" double hda_pcg_iteration_bytes(hda_csr_t A) { return A ? pcg_iteration_bytes(A->get()) : 0.0; }

extern "C" int hda_format_bytes(hda_csr_t A, hda_amg_t amg, double *pcg_iteration, double *vcycle, double *spmv, int *coded)
{
   HDA_TRY
   const DCsr &m = A->get();
   if (pcg_iteration) *pcg_iteration = pcg_iteration_bytes(m, true);
   if (vcycle) *vcycle = amg ? amg->pc.amg->vcycle_bytes(true) : 0.0;
   if (spmv) *spmv = matrix_stream_bytes(m, true) + rowptr_stream_bytes(m, true) + 8.0 * m.ncols + 8.0 * m.nrows;
   // storage form the products of A use: 0 plain CSR, 1 entry-coded stencil operator, 2 row-class coded, 3 windowed CSR,
   // 4 value-coded, 5 value-coded + windowed
   if (coded) *coded = (m.coded == 1) ? (m.rowcoded == 1 ? 2 : 1) : (m.coded == 2) ? (m.win == 1 ? 5 : 4) : (m.win == 1 ? 3 : 0);
   HDA_CATCH
}

extern "C" int hda_csr_form(hda_csr_t A, int nown, int *info)
{
   HDA_TRY
   if (!A || !info) { g_err = "hda_csr_form: null matrix or info"; return HDA_ERR_ARG; }
   const DCsr &m = A->get();
   if (nown > m.ncols) { g_err = "hda_csr_form: nown must lie in [0, ncols] (or be negative: the whole product)"; return HDA_ERR_ARG; }
   spmv_form_info(m, nown, info);
   HDA_CATCH
}

extern "C" int hda_spmv_mode(hda_csr_t A, int mode, int nown, double alpha, double beta, const double *x, const double *yin, const double *b,
                             const double *dinv, const double *w, const double *dinv2, double *y, double *y2, double *dot, int *epilogue_taken)
{
   HDA_TRY
   auto bad = [](const char *msg) { g_err = std::string("hda_spmv_mode: ") + msg; return HDA_ERR_ARG; };
   if (!A) return bad("null matrix");
   const DCsr &m   = A->get();
   const bool  jac = mode == HDA_SPMV_JACOBI || mode == HDA_SPMV_JACOBI_DOT;
   if (mode < HDA_SPMV_PLAIN || mode > HDA_SPMV_SCALED_COPY) return bad("unknown mode");
   if (nown > m.ncols) return bad("nown must lie in [0, ncols] (or be negative: the whole product)");
   if (!x || !y) return bad("x and y are required");
   if (mode == HDA_SPMV_PLAIN && beta != 0.0 && !yin) return bad("beta != 0 reads yin");
   if (mode == HDA_SPMV_PLAIN_DOT && !w) return bad("the fused dot reads w");
   if ((mode == HDA_SPMV_RESID || jac) && !b) return bad("this mode reads b");
   if (jac && !dinv) return bad("the Jacobi sweep reads dinv");
   if (jac && m.nrows > m.ncols) return bad("the Jacobi sweep reads x[i] for every row i: nrows <= ncols");
   if ((mode == HDA_SPMV_PLAIN_DOT || mode == HDA_SPMV_JACOBI_DOT) && !dot) return bad("a fused dot needs dot");
   if (mode == HDA_SPMV_SCALED_COPY && (!dinv2 || !y2)) return bad("the scaled copy needs dinv2 and y2");
   const size_t   nr = (size_t)m.nrows, nc = (size_t)m.ncols;
   DArray<double> dx, dyin, db, ddinv, dw, ddinv2, dy, dy2;
   dx.upload(x, nc);
   dy.upload(y, nr);
   const bool in_place = yin == y; // yin aliases y on the device as well
   if (mode == HDA_SPMV_PLAIN && yin && !in_place) dyin.upload(yin, nr);
   if (b) db.upload(b, nr);
   if (dinv) ddinv.upload(dinv, nr);
   if (w) dw.upload(w, nr);
   if (mode == HDA_SPMV_SCALED_COPY)
   {
      ddinv2.upload(dinv2, nr);
      dy2.upload(y2, nr); // rows the product leaves alone come back as they were given
   }
   const double *pyin = (mode != HDA_SPMV_PLAIN || !yin) ? nullptr : in_place ? dy.data() : dyin.data();
   double        d    = 0.0;
   bool          taken = false;
   spmv_test_mode(m, mode, nown, alpha, beta, dx.data(), pyin, db.data(), ddinv.data(), dw.data(), ddinv2.data(), dy.data(), dy2.data(), &d, &taken);
   dy.download(y, nr);
   if (mode == HDA_SPMV_SCALED_COPY) dy2.download(y2, nr);
   if (dot) *dot = d;
   if (epilogue_taken) *epilogue_taken = taken;
   HDA_CATCH
}

// Borrowed seam views of a HYPREDRV object whose solver is set up: its level-0 operator (with the right-hand side and
// the ghost refresh plan of a row block) and its BoomerAMG hierarchy.  bench.py measures the object the API
// built, not a second copy.  Valid until LinearSolverDestroy / PreconDestroy; release with hda_csr_destroy / hda_amg_destroy.
extern "C" int hda_borrow_hypredrv(void *hypredrv, hda_csr_t *A, hda_amg_t *amg)
{
   HDA_TRY
   const DCsr     *m    = nullptr;
   const HaloPlan *halo = nullptr;
   const double   *rhs  = nullptr;
   Amg            *g    = nullptr;
   HDA_REQUIRE(hypredrv_peek(hypredrv, &m, &halo, &rhs, &g) && m, "hda_borrow_hypredrv: the object has no matrix yet");
   if (A)
   {
      auto v      = std::make_unique<hda_csr_s>();
      v->borrowed = true;
      v->ref      = m;
      v->rhs_ref  = rhs;
      v->halo     = halo;
      *A          = v.release();
   }
   if (amg)
   {
      HDA_REQUIRE(g, "hda_borrow_hypredrv: the preconditioner is not a set-up BoomerAMG hierarchy");
      auto h = std::make_unique<hda_amg_s>();
      h->pc.amg  = g;
      h->pc.kind = Precond::AMG;
      *amg   = h.release();
   }
   HDA_CATCH
}

// Raw device buffers from the library's allocator: what a caller without a HIP client of its own (the Python binding's DeviceBuffer)
// hands to the IJ calls of an object initialised with HYPRE_MEMORY_DEVICE.  Copies run on the library stream and are complete on return.
extern "C" int hda_dev_alloc(int64_t bytes, void **ptr)
{
   HDA_TRY
   HDA_REQUIRE(bytes >= 0 && ptr, "hda_dev_alloc: bytes >= 0 and ptr are required");
   *ptr = pool_alloc((size_t)std::max<int64_t>(bytes, 1));
   HDA_CATCH
}
extern "C" int hda_dev_free(void *ptr)
{
   if (!ptr) return HDA_OK;
   HDA_TRY
   Context::get().sync();
   pool_free(ptr);
   HDA_CATCH
}
extern "C" int hda_dev_upload(void *dst, const void *host, int64_t bytes)
{
   HDA_TRY
   HDA_REQUIRE(bytes >= 0 && (bytes == 0 || (dst && host)), "hda_dev_upload: null buffer");
   if (bytes) HDA_HIP(hipMemcpyAsync(dst, host, (size_t)bytes, hipMemcpyHostToDevice, Context::get().stream));
   Context::get().sync();
   HDA_CATCH
}
extern "C" int hda_dev_download(void *host, const void *src, int64_t bytes)
{
   HDA_TRY
   HDA_REQUIRE(bytes >= 0 && (bytes == 0 || (src && host)), "hda_dev_download: null buffer");
   download_sync(host, src, (size_t)bytes);
   HDA_CATCH
}

// Borrowed view of the operator behind an assembled HYPRE_IJMatrix (columns >= its local column count are ghosts, in the order of
// hda_ij_ghost_gids).  Valid until the handle is destroyed; release with hda_csr_destroy.
extern "C" int hda_borrow_ij_matrix(void *ij_matrix, hda_csr_t *out)
{
   HDA_TRY
   auto *m = (hypre_IJMatrix_struct *)ij_matrix;
   HDA_REQUIRE(m && out && m->assembled, "hda_borrow_ij_matrix: an assembled IJ matrix is required");
   auto v      = std::make_unique<hda_csr_s>();
   v->borrowed = true;
   v->ref      = &m->A;
   *out        = v.release();
   HDA_CATCH
}
// ascending global ids of its ghost columns: *n of them, the first min(*n, cap) written to gids (may be NULL with cap 0)
extern "C" int hda_ij_ghost_gids(void *ij_matrix, long long *gids, int cap, int *n)
{
   auto *m = (hypre_IJMatrix_struct *)ij_matrix;
   if (!m || !n) { g_err = "hda_ij_ghost_gids: null argument"; return HDA_ERR_ARG; }
   *n = (int)m->ghost_gids.size();
   for (int q = 0; q < *n && q < cap && gids; q++) gids[q] = m->ghost_gids[(size_t)q];
   return HDA_OK;
}

// the last HYPRE_IJMatrixAssemble of an object initialised with HYPRE_MEMORY_DEVICE on this rank: out[0] path (0 nothing stacked, 1 the
// stack was a CSR block, 2 sort + run reduction), [1] entries stacked, [2] entries after merging, [3] ms of the sort, [4] ms of the
// run-reduce kernel (path 2; stream time)
extern "C" int hda_ij_last_assembly(double out[5])
{
   if (!out) { g_err = "hda_ij_last_assembly: null argument"; return HDA_ERR_ARG; }
   const IjAssemblyStats &s = ij_assembly_stats();
   out[0] = s.path; out[1] = (double)s.stacked; out[2] = (double)s.merged; out[3] = s.sort_ms; out[4] = s.reduce_ms;
   return HDA_OK;
}

// The library's halo-plan construction without its device half, for the CPU (gloo) test of the N > 1 path: collective over the
// communicator joined with HYPREDRV_AMD_CommInitCallbacks.  part: row starts of every rank (world + 1 entries); ghost_gids:
// ascending global ids of this rank's ghost columns.  Outputs: send_counts / recv_counts (world entries each), send_idx (the
// owned rows to pack, grouped by ascending destination; at most send_cap entries are written), *send_total.
extern "C" int hda_halo_plan_host(int nloc, const long long *part, const long long *ghost_gids, int nghost, int *send_counts,
                                  int *recv_counts, int *send_idx, int send_cap, int *send_total)
{
   try
   {
      Comm                  &cm = Comm::world();
      std::vector<long long> pv(part, part + cm.size + 1), gv(ghost_gids, ghost_gids + std::max(nghost, 0));
      std::vector<int>       sc, rc, idx;
      halo_plan_host(nloc, pv, gv, sc, rc, idx);
      for (int p = 0; p < cm.size; p++) { send_counts[p] = sc[(size_t)p]; recv_counts[p] = rc[(size_t)p]; }
      for (size_t q = 0; q < idx.size() && (int)q < send_cap; q++) send_idx[q] = idx[q];
      if (send_total) *send_total = (int)idx.size();
   }
   catch (const std::exception &e)
   {
      g_err = e.what();
      return HDA_ERR_RUNTIME;
   }
   return HDA_OK;
}

extern "C" int hda_probe_add(hda_csr_t A, int mode, int *id)
{
   HDA_TRY
   HDA_REQUIRE(A && mode >= 0 && mode <= 2, "probe: matrix and mode 0 plain, 1 residual, 2 Jacobi");
   const int k = spmv_probe_add(&A->get(), mode);
   if (id) *id = k;
   HDA_CATCH
}
extern "C" int hda_probe_read_id(int id, double *avg_ms, int *count)
{
   HDA_TRY
   spmv_probe_read(id, avg_ms, count);
   HDA_CATCH
}
// rank-to-rank traffic since the last reset: [0] device all-reduces, [1] halo exchanges (neighbour send/recv groups),
// [2] doubles all-reduced, [3] doubles sent in halo exchanges, [4] exchanges whose transfer ran under a product kernel
extern "C" int hda_comm_stats(double out[5], int reset)
{
   Comm &cm = Comm::world();
   if (out)
   {
      out[0] = (double)cm.stats.allreduce; out[1] = (double)cm.stats.exchange; out[2] = (double)cm.stats.allreduce_doubles;
      out[3] = (double)cm.stats.exchange_doubles; out[4] = (double)cm.stats.overlapped;
   }
   if (reset) cm.stats = Comm::Stats();
   return HDA_OK;
}
extern "C" const char *hda_comm_name(void) { return Comm::world().name(); }
extern "C" int hda_comm_size(void) { return Comm::world().size; }

extern "C" int hda_probe_spmv(hda_csr_t A, int mode)
{
   HDA_TRY
   HDA_REQUIRE(mode >= 0 && mode <= 2, "probe mode: 0 plain, 1 residual, 2 Jacobi");
   spmv_probe_clear();
   if (A) spmv_probe_add(&A->get(), mode);
   HDA_CATCH
}
extern "C" int hda_probe_read(double *avg_ms, int *count)
{
   HDA_TRY
   spmv_probe_read(0, avg_ms, count);
   HDA_CATCH
}

extern "C" int hda_check_row_total(long long nrows, int row_len)
{
   HDA_TRY
   HDA_REQUIRE(nrows >= 0 && nrows < (1LL << 31) && row_len >= 0, "bad arguments");
   DArray<int>      len((size_t)std::max<long long>(nrows, 1));
   std::vector<int> h((size_t)nrows, row_len);
   if (nrows) len.upload(h.data(), (size_t)nrows);
   require_int32_total((long)nrows, len.data(), "row block");
   HDA_CATCH
}

extern "C" int hda_memory_stats(double *in_use, double *peak)
{
   if (in_use) *in_use = (double)pool_bytes_in_use();
   if (peak) *peak = (double)pool_bytes_peak();
   return HDA_OK;
}

extern "C" double hda_memory_cached(void) { return (double)pool_bytes_cached(); }
extern "C" int    hda_memory_driver_stats(double out[3], int reset)
{
   HDA_TRY
   pool_driver_stats(out, reset != 0);
   HDA_CATCH
}
extern "C" int    hda_memory_trim(void)
{
   HDA_TRY
   pool_trim();
   HDA_CATCH
}

extern "C" int hda_comm_selftest(void)
{
   HDA_TRY
   Comm &cm = Comm::world();
   // device all-reduce of [rank+1, 1]
   DArray<double> d(2);
   double         hv[2] = {(double)cm.rank + 1.0, 1.0};
   d.upload(hv, 2);
   cm.allreduce_sum_dev(d.data(), 2);
   d.download(hv, 2);
   HDA_REQUIRE(hv[0] == 0.5 * cm.size * (cm.size + 1) && hv[1] == (double)cm.size, "device all-reduce gave a wrong sum");
   // host all-reduce (max of rank)
   long long m[1] = {cm.rank};
   cm.allreduce_host(m, 1, 1);
   HDA_REQUIRE(m[0] == cm.size - 1, "host all-reduce(max) is wrong");
   // host all-to-all: rank r sends (r*100 + p) to p
   std::vector<long long> snd((size_t)cm.size), rcv((size_t)cm.size);
   std::vector<long>      eight((size_t)cm.size, 8);
   for (int p = 0; p < cm.size; p++) snd[(size_t)p] = cm.rank * 100 + p;
   cm.alltoallv_host(snd.data(), eight.data(), rcv.data(), eight.data());
   for (int p = 0; p < cm.size; p++) HDA_REQUIRE(rcv[(size_t)p] == p * 100 + cm.rank, "host all-to-all is wrong");
   // device neighbour exchange: one double to every other rank
   std::vector<int> cnt((size_t)cm.size, 1);
   cnt[(size_t)cm.rank] = 0;
   const int      np = cm.size - 1;
   DArray<double> sb((size_t)std::max(np, 1)), rb((size_t)std::max(np, 1));
   std::vector<double> hs((size_t)std::max(np, 1), (double)cm.rank), hr((size_t)std::max(np, 1), -1.0);
   sb.upload(hs.data(), hs.size());
   rb.upload(hr.data(), hr.size());
   cm.exchange_dev(sb.data(), cnt.data(), rb.data(), cnt.data());
   rb.download(hr.data(), hr.size());
   for (int p = 0, q = 0; p < cm.size; p++)
      if (p != cm.rank) { HDA_REQUIRE(hr[(size_t)q] == (double)p, "device exchange is wrong"); q++; }
   HDA_CATCH
}
