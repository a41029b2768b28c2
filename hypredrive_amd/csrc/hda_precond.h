// hda_precond.h -- one preconditioner of any kind, as both C APIs hold it (hda_amg_s in hda_capi.hip, hypre_Solver_struct in
// hda_hypre.h).  The switches below are the one place that knows the six calling conventions; everything else a kind offers
// (factors, levels, setup times) stays on its class and is reached through the typed pointer.
#pragma once

#include "hda_krylov.h"

namespace hda {

struct Precond {
   enum Kind { NONE, AMG, ILU, MGR, SCHWARZ, AMS, FSAI };
   Kind                     kind = NONE;  // set together with the pointer of that kind
   Amg                     *amg  = nullptr; // the hierarchy: owned_amg.get(), or borrowed from a HYPREDRV object
   std::unique_ptr<Amg>     owned_amg;
   std::unique_ptr<Ilu>     ilu;
   std::unique_ptr<Mgr>     mgr;
   std::unique_ptr<Schwarz> schwarz;
   std::unique_ptr<Ams>     ams;
   std::unique_ptr<Fsai>    fsai;
   DArray<double>           r, c; // residual and correction of the stationary kinds

   // iterations x += M^-1 (b - A x) of one solve
   int iterations() const
   {
      switch (kind)
      {
         case AMG: return std::max(amg->prm.max_iter, 1);
         case ILU: return std::max(ilu->prm.max_iter, 1);
         case MGR: return std::max(mgr->prm.max_iter, 1);
         case SCHWARZ: return std::max(schwarz->prm.max_iter, 1);
         case AMS: return std::max(ams->prm.max_iter, 1);
         case FSAI: return std::max(fsai->prm.max_iter, 1);
         default: return 0;
      }
   }
   // that solve; zero_guess: x counts as zero and is not read.  halo: ghost refresh of x (A a row block), x then has vec_len(A) entries
   void solve(const DCsr &A, const HaloPlan *halo, const double *b, double *x, bool zero_guess)
   {
      switch (kind)
      {
         case AMG: zero_guess ? amg->apply(b, x, -1) : amg->solve(b, x); break; // (from a zero guess: ONE cycle, as a Krylov loop takes it)
         case MGR: mgr->solve(b, x, zero_guess); break;
         case ILU: stationary_solve(*ilu, A, halo, b, x, zero_guess, iterations(), r, c); break;
         case SCHWARZ: stationary_solve(*schwarz, A, halo, b, x, zero_guess, iterations(), r, c); break;
         case FSAI: stationary_solve(*fsai, A, halo, b, x, zero_guess, iterations(), r, c); break;
         case AMS: stationary_solve(*ams, A, halo, b, x, zero_guess, 1, r, c); break; // (its max_iter cycles run inside one application)
         default: throw Error("no preconditioner has been set up on this handle");
      }
   }
   // length of the vectors handed to solve()
   size_t vec_len(const DCsr &A) const
   {
      return kind == AMG ? amg->vec_len0() : kind == MGR ? mgr->vec_len0() : (size_t)std::max(std::max(A.ncols, A.nrows), 1);
   }
   // the preconditioner of one of this library's Krylov loops on A (A, halo and this object outlive it)
   PrecondFn as_fn(const DCsr &A, const HaloPlan *halo)
   {
      if (kind == AMG) return [this](const double *rr, double *zz, int slot) { amg->apply_offering(rr, zz, slot); };
      return [this, &A, halo](const double *rr, double *zz, int slot) {
         solve(A, halo, rr, zz, true);
         if (slot >= 0) dot(A.nrows, rr, zz, slot);
      };
   }
};

} // namespace hda
