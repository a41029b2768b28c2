// hda_ams.hip -- auxiliary-space Maxwell preconditioner (AMS, Hiptmair-Xu) for definite curl-curl + mass operators discretised with
// lowest-order Nedelec elements, as hypredrv_AMSCreate configures hypre's (reference src/internal/ams.c:37-63, :78-102).  hypre is not
// part of the reference tree, so the algorithm is restated (tests/ams_reference.py is the same definition on the
// host).  PARITY UNPINNED against hypre: no reference output for AMS exists.
//
//   inputs   A (n_e x n_e), the discrete gradient G (n_e x n_v), vertex coordinates c_0 .. c_{d-1} (d = dimension, 2 or 3)
//   Pi       n_e x d n_v: entry (i, j) of G becomes the d entries (i, d j + k) = (|G_ij| * 0.5) * g_k[i], g_k = G c_k
//   A_G      G^T A G, A_Pi = Pi^T A Pi: structural products, nothing dropped; a row without a non-zero value becomes a unit diagonal
//   B_G      BoomerAMG on A_G (beta_* keys, one function), B_Pi on A_Pi (alpha_* keys, d interleaved functions); one V(1,1) each
//   apply    z = 0; per character of the cycle string  0: relax_times sweeps z += w (r - A z) / l1(A)
//                                                      1: z += G B_G (G^T (r - A z))      2: z += Pi B_Pi (Pi^T (r - A z))
//
// G^T and Pi^T are explicit CSR matrices, so every product of the cycle is a row gather: no atomics, bitwise reproducible.  An
// application launches the existing product, sweep and V-cycle kernels on vectors allocated by the setup.
#include "hda_amg.h"

#include <algorithm>

namespace hda {

#define STREAM (Context::get().stream)

namespace {

// entry q of Pi: entry e = q / d of G, component k = q % d; the row of e by bisection of G's row pointers
__global__ __launch_bounds__(256) void k_ams_pi(int nrows, int nnz, int d, const int *__restrict__ rp, const int *__restrict__ cj,
                                                const double *__restrict__ gv, const double *__restrict__ g0, const double *__restrict__ g1,
                                                const double *__restrict__ g2, int *__restrict__ pcol, double *__restrict__ pval)
{
   const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
   if (q >= (long long)nnz * d) return;
   const int e = (int)(q / d), k = (int)(q - (long long)e * d);
   int       a = 0, b = nrows; // rp[a] <= e < rp[b]
   while (b - a > 1)
   {
      const int m = (a + b) >> 1;
      if (rp[m] <= e) a = m;
      else b = m;
   }
   const double *g = (k == 0) ? g0 : (k == 1) ? g1 : g2;
   pcol[q]         = d * cj[e] + k;
   pval[q]         = (fabs(gv[e]) * 0.5) * g[a];
}
__global__ __launch_bounds__(256) void k_ams_pi_rowptr(int nrows, int d, const int *__restrict__ rp, int *__restrict__ prp)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i <= nrows) prp[i] = d * rp[i];
}

// zero-row repair: a row with no entry or with zero values only takes one entry
__global__ __launch_bounds__(256) void k_ams_fix_count(int n, const int *__restrict__ rp, const double *__restrict__ v, int *__restrict__ len)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   bool any = false;
   for (int k = rp[i]; k < rp[i + 1]; k++) any = any || (v[k] != 0.0);
   len[i] = any ? rp[i + 1] - rp[i] : 1;
}
__global__ __launch_bounds__(256) void k_ams_fix_fill(int n, const int *__restrict__ rp, const int *__restrict__ cj, const double *__restrict__ v,
                                                      const int *__restrict__ len, const int *__restrict__ nrp, int *__restrict__ ncj,
                                                      double *__restrict__ nv, int *__restrict__ repaired)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   int  o   = nrp[i];
   bool any = (len[i] > 1); // (a row of length one may be a kept row or a repaired one)
   for (int k = rp[i]; k < rp[i + 1] && !any; k++) any = (v[k] != 0.0);
   if (!any)
   {
      ncj[o]      = i;
      nv[o]       = 1.0;
      repaired[i] = 1;
      return;
   }
   repaired[i] = 0;
   for (int k = rp[i]; k < rp[i + 1]; k++, o++)
   {
      ncj[o] = cj[k];
      nv[o]  = v[k];
   }
}

int last_entry(const DArray<int> &scan, size_t n)
{
   int v = 0;
   download_sync(&v, scan.data() + n, sizeof(int));
   return v;
}

} // namespace

// ---- the free parameters of the definition: what hypre's AMS fixes inside and ams.c does not set
AmgParams ams_subspace_amg(const AmsAmgOptions &o, int num_functions)
{
   AmgParams p;
   p.coarsen_type   = o.coarsen_type;
   p.agg_num_levels = o.agg_levels;
   p.relax_down = p.relax_up = o.relax_type;
   p.strong_th      = o.strength_threshold;
   p.interp_type    = o.interp_type;
   p.pmax           = o.pmax;
   p.relax_coarse   = o.coarse_relax_type;
   p.num_functions  = num_functions;
   p.sweeps_down = p.sweeps_up = p.sweeps_coarse = 1; // V(1,1), one sweep on the coarsest level
   p.max_iter        = 1;
   p.tol             = 0.0;
   // free parameters
   p.max_levels      = 25;
   p.max_coarse_size = 9;
   p.min_coarse_size = 2;
   p.max_row_sum     = 0.9;
   p.agg_interp_type = 4; // multipass
   p.agg_num_paths   = 1;
   p.trunc_factor    = 0.0;
   return p;
}

const char *ams_cycle_string(int cycle_type)
{
   switch (cycle_type)
   {
      case 1: return "01210";
      case 3: return "02120";
      case 5: return "0102010";
      case 7: return "0201020";
      default: return nullptr;
   }
}

std::string ams_refusal(const AmsParams &p)
{
   if (!ams_cycle_string(p.cycle_type))
      return "AMS: cycle_type " + std::to_string(p.cycle_type) +
             " is not implemented on MI355X; the multiplicative cycles 1, 3, 5 and 7 are (additive and component-wise cycles are not)";
   if (p.relax_type != 1)
      return "AMS: relax_type " + std::to_string(p.relax_type) + " is not implemented on MI355X; 1 (l1-Jacobi) is";
   if (p.dimension != 2 && p.dimension != 3) return "AMS: dimension " + std::to_string(p.dimension) + " is not valid (2 or 3)";
   if (p.tolerance != 0.0) return "AMS: tolerance != 0 (a residual test inside the preconditioner) is not implemented; max_iter fixed cycles are";
   if (p.max_iter < 1) return "AMS: max_iter must be >= 1";
   if (p.relax_times < 1) return "AMS: relax_times must be >= 1";
   if (p.alpha.agg_num_levels > 0)
      return "AMS: alpha_agg_levels " + std::to_string(p.alpha.agg_num_levels) +
             " is not implemented: aggressive levels with num_functions > 1 are not built (set alpha_agg_levels: 0)";
   return "";
}

void ams_build_pi(const DCsr &G, int d, const double *const g[3], DCsr &Pi)
{
   HDA_REQUIRE(d == 2 || d == 3, "AMS: dimension must be 2 or 3");
   HDA_REQUIRE((long long)G.nnz * d < 2147483647LL && (long long)G.ncols * d < 2147483647LL, "AMS: Pi outgrows 32-bit indices");
   Pi       = DCsr();
   Pi.nrows = G.nrows;
   Pi.ncols = d * G.ncols;
   Pi.nnz   = d * G.nnz;
   Pi.rowptr.alloc((size_t)Pi.nrows + 1);
   Pi.col.alloc((size_t)std::max(Pi.nnz, 1));
   Pi.val.alloc((size_t)std::max(Pi.nnz, 1));
   k_ams_pi_rowptr<<<ceil_div(G.nrows + 1, 256), 256, 0, STREAM>>>(G.nrows, d, G.rowptr.data(), Pi.rowptr.data());
   if (Pi.nnz)
      k_ams_pi<<<ceil_div(Pi.nnz, 256), 256, 0, STREAM>>>(G.nrows, G.nnz, d, G.rowptr.data(), G.col.data(), G.val.data(), g[0], g[1],
                                                         d > 2 ? g[2] : g[1], Pi.col.data(), Pi.val.data());
}

int ams_fix_zero_rows(DCsr &C)
{
   HDA_REQUIRE(C.nrows == C.ncols, "AMS: the zero-row repair needs a square matrix");
   const int n = C.nrows;
   if (n == 0) return 0;
   DArray<int> len((size_t)n + 1), nrp((size_t)n + 1), rep((size_t)n + 1);
   len.zero();
   k_ams_fix_count<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, C.rowptr.data(), C.val.data(), len.data());
   require_int32_total(n, len.data(), "AMS subspace matrix");
   exclusive_scan(n, len.data(), nrp.data(), nullptr);
   const int      nnz = last_entry(nrp, (size_t)n);
   DArray<int>    ncj((size_t)std::max(nnz, 1));
   DArray<double> nv((size_t)std::max(nnz, 1));
   rep.zero();
   k_ams_fix_fill<<<ceil_div(n, 256), 256, 0, STREAM>>>(n, C.rowptr.data(), C.col.data(), C.val.data(), len.data(), nrp.data(), ncj.data(),
                                                       nv.data(), rep.data());
   exclusive_scan(n, rep.data(), len.data(), nullptr);
   const int fixed = last_entry(len, (size_t)n);
   C.rowptr        = std::move(nrp);
   C.col           = std::move(ncj);
   C.val           = std::move(nv);
   C.nnz           = nnz;
   C.reset_plan();
   return fixed;
}

static void ams_check_amg(const AmgParams &o, int num_functions, const char *space)
{ // every refusal of the BoomerAMG setup that one of the seven keys of a subspace can cause, under the AMS key that carried the value
  // (strength_threshold and Pmax are refused by nothing); anything else reaches the catch of Ams::setup with the space's name only
   const std::string s = std::string("AMS: ") + space;
   if (!amg_coarsen_type_built(o.coarsen_type)) throw Error(s + "_coarsen_type: " + amg_coarsen_refusal(o.coarsen_type));
   if (o.coarsen_type != 8 && o.coarsen_type != 10 && num_functions > 1)
      throw Error(s + "_coarsen_type " + std::to_string(o.coarsen_type) + ": coarsening types cljp, rs and falgout are implemented on scalar problems only");
   if (o.coarsen_type != 8 && o.coarsen_type != 10 && o.agg_num_levels > 0)
      throw Error(s + "_agg_levels " + std::to_string(o.agg_num_levels) + ": coarsening types cljp, rs and falgout are implemented without aggressive levels");
   if (!amg_interp_type_built(o.interp_type)) throw Error(s + "_interp_type: " + amg_interp_refusal(o.interp_type));
   if (o.interp_type == 4 && num_functions > 1)
      throw Error(s + "_interp_type 4: multipass interpolation is implemented on a scalar problem only");
   if (!amg_relax_type_built(o.relax_down) || !amg_relax_type_built(o.relax_up))
      throw Error(s + "_relax_type " + std::to_string(amg_relax_type_built(o.relax_down) ? o.relax_up : o.relax_down) + ": " + amg_relax_refusal(false));
   if (!amg_relax_type_built(o.relax_coarse, true))
      throw Error(s + "_coarse_relax_type " + std::to_string(o.relax_coarse) + ": " + amg_relax_refusal(true));
}

void Ams::setup(const DCsr &A_, const DCsr &G_, const double *const coords[3], const AmsParams &p)
{
   const std::string why = ams_refusal(p);
   if (!why.empty()) throw Error(why);
   HDA_REQUIRE(A_.nrows == A_.ncols, "AMS: the operator must be square");
   HDA_REQUIRE(G_.nrows == A_.nrows, "AMS: the discrete gradient needs one row per row of the operator");
   for (int k = 0; k < p.dimension; k++) HDA_REQUIRE(coords[k] || G_.ncols == 0, "AMS: a coordinate vector is missing");
   ams_check_amg(p.beta, 1, "beta");
   ams_check_amg(p.alpha, p.dimension, "alpha");
   prm = p;
   prm.alpha.num_functions = p.dimension; // the function of column d j + k is k: the interleaved default
   prm.beta.num_functions  = 1;
   A   = &A_;
   G   = DCsr(); // a copy: the caller's gradient may go before this object does
   G.nrows = G_.nrows; G.ncols = G_.ncols; G.nnz = G_.nnz;
   G.rowptr.copy_from(G_.rowptr); G.col.copy_from(G_.col); G.val.copy_from(G_.val);
   n_e = A_.nrows;
   n_v = G_.ncols;
   const int d  = p.dimension;
   auto      t0 = std::chrono::steady_clock::now();
   auto      ms = [&]() {
      Context::get().sync();
      auto         t1 = std::chrono::steady_clock::now();
      const double v  = std::chrono::duration<double, std::milli>(t1 - t0).count();
      t0              = t1;
      return v;
   };

   // ---- Pi from G and g_k = G c_k
   {
      DArray<double> g[3];
      const double  *gp[3] = {nullptr, nullptr, nullptr};
      for (int k = 0; k < d; k++)
      {
         g[k].alloc((size_t)std::max(n_e, 1));
         if (n_e) spmv(G_, 1.0, coords[k], 0.0, nullptr, g[k].data());
         gp[k] = g[k].data();
      }
      ams_build_pi(G_, d, gp, Pi);
      Context::get().sync(); // (g leaves scope: the pool may hand its blocks to the next request, which is later on the same stream anyway)
   }
   transpose(G_, GT);
   transpose(Pi, PiT);
   setup_ms[0] = ms();

   // ---- Galerkin products and their repair
   amg_rap(A_, G_, GT, A_G);
   amg_rap(A_, Pi, PiT, A_Pi);
   fixed_rows[0] = ams_fix_zero_rows(A_G);
   fixed_rows[1] = ams_fix_zero_rows(A_Pi);
   setup_ms[1]   = ms();

   // ---- the subspace solvers
   auto build = [&](std::unique_ptr<Amg> &B, const DCsr &M, const AmgParams &o, int nf, const char *space) {
      B = std::make_unique<Amg>(o);
      try
      {
         B->setup(M);
      }
      catch (const std::exception &e)
      {
         throw Error(std::string("AMS: ") + space + "_* (BoomerAMG on " + (nf == 1 ? "G^T A G" : "Pi^T A Pi") + "): " + e.what());
      }
   };
   build(B_G, A_G, prm.beta, 1, "beta");
   setup_ms[2] = ms();
   build(B_Pi, A_Pi, prm.alpha, d, "alpha");
   setup_ms[3] = ms();

   // ---- smoother divisors and the vectors of the cycle
   dinv.alloc((size_t)std::max(n_e, 1));
   {
      DArray<double> l1((size_t)std::max(n_e, 1));
      l1_row_norms(A_, 1, l1.data());
      make_dinv(n_e, l1.data(), p.relax_weight, dinv.data());
      Context::get().sync();
   }
   t.alloc((size_t)std::max(n_e, 1));
   z2.alloc((size_t)std::max(std::max(n_e, A_.ncols), 1));
   const size_t lg = std::max<size_t>(std::max<size_t>(B_G->vec_len0(), (size_t)n_v), 1);
   const size_t lp = std::max<size_t>(std::max<size_t>(B_Pi->vec_len0(), (size_t)d * n_v), 1);
   rg.alloc(lg); eg.alloc(lg); rp.alloc(lp); ep.alloc(lp);
   rg.zero(); eg.zero(); rp.zero(); ep.zero();
   spmv_prepare(G); spmv_prepare(GT); spmv_prepare(PiT); spmv_prepare(Pi);
   Context::get().sync();
}

// z = M r from z = 0 (r and z must not alias; z needs the room of a level-0 vector of A)
void Ams::apply(const double *r, double *z)
{
   if (n_e == 0) return;
   const char *cyc   = ams_cycle_string(prm.cycle_type);
   int         zeros = 0;
   for (const char *c = cyc; *c; c++) zeros += (*c == '0');
   // every sweep but the first (which writes dinv .* r) moves the iterate to the other buffer: start where the last one ends in z
   const long long swaps = (long long)prm.max_iter * zeros * prm.relax_times - 1;
   double         *cur = (swaps % 2 == 0) ? z : z2.data(), *alt = (cur == z) ? z2.data() : z;
   bool            zero = true;
   for (int it = 0; it < prm.max_iter; it++)
      for (const char *c = cyc; *c; c++)
      {
         if (*c == '0')
         {
            for (int s = 0; s < prm.relax_times; s++)
            {
               if (zero)
               { // r - A 0 = r exactly
                  jacobi_zero_guess(n_e, dinv.data(), r, cur);
                  zero = false;
                  continue;
               }
               jacobi(*A, dinv.data(), r, cur, alt, -1);
               std::swap(cur, alt);
            }
            continue;
         }
         residual(*A, cur, r, t.data());
         if (*c == '1')
         {
            spmv(GT, 1.0, t.data(), 0.0, nullptr, rg.data());
            B_G->apply(rg.data(), eg.data());
            spmv(G, 1.0, eg.data(), 1.0, cur, cur);
         }
         else
         {
            spmv(PiT, 1.0, t.data(), 0.0, nullptr, rp.data());
            B_Pi->apply(rp.data(), ep.data());
            spmv(Pi, 1.0, ep.data(), 1.0, cur, cur);
         }
      }
   HDA_REQUIRE(cur == z, "AMS: the cycle did not end in the output vector");
}

double Ams::apply_bytes() const
{ // CSR figure of one application: the sweeps and residuals over A, the four transfers, the two V-cycles, per cycle character
   auto   mat = [](const DCsr &M) { return 12.0 * M.nnz + 4.0 * (M.nrows + 1.0) + 8.0 * M.ncols + 8.0 * M.nrows; };
   double b   = 0.0;
   for (const char *c = ams_cycle_string(prm.cycle_type); c && *c; c++)
   {
      if (*c == '0') b += prm.relax_times * (mat(*A) + 16.0 * n_e);
      else if (*c == '1') b += mat(*A) + 8.0 * n_e + mat(GT) + mat(G) + 8.0 * n_e + B_G->vcycle_bytes();
      else b += mat(*A) + 8.0 * n_e + mat(PiT) + mat(Pi) + 8.0 * n_e + B_Pi->vcycle_bytes();
   }
   return b * prm.max_iter;
}

} // namespace hda
