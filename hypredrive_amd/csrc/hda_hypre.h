// hda_hypre.h -- the objects behind the HYPRE_* handles declared in include/HYPRE.h.
#pragma once

#include "../../include/HYPRE.h"
#include "hda_precond.h"

#include <memory>
#include <string>

struct hypre_IJVector_struct {
   MPI_Comm             comm = MPI_COMM_WORLD;
   long long            jlower = 0, jupper = -1;
   int                  nloc   = 0;
   bool                 initialized = false, assembled = false;
   // what the last Initialize_v2 was given: where the CALLER's idx / value arrays of Set / AddTo / GetValues live (the vector's own
   // data is HBM resident either way).  DEVICE: every call is applied to d at once (hda_ij_device.hip), stage stays empty
   HYPRE_MemoryLocation location = HYPRE_MEMORY_HOST;
   std::vector<double>  stage;       // host values until Assemble
   hda::DArray<double>  d;           // owned entries (+ optional ghost room) in HBM
   size_t               capacity = 0; // doubles available behind data()
   double              *view = nullptr; // non-owning alias of somebody else's HBM buffer
   std::vector<double>  host_mirror; // backing store for "get values" pointers
   // Modification counter.  Everything that can change the values bumps it: the mutable accessor data() (whoever takes it may
   // write), the value setters, Assemble, a fill or a copy into the vector, and handing the handle to a caller
   // (HYPREDRV_LinearSystemGetSolution / GetRHS).  The library's read paths take cdata(), which leaves it alone.  Two facts are
   // kept per counter value and are void as soon as it moves:
   //   zero_at: the vector was filled by the library's own zero fill (or copied from a vector in that state) and nothing has
   //            written it since -- x = 0 exactly, so b - A x is b bit for bit
   //   bb_at:   <v,v> as the dot kernel and its finalize computed it (bb), so that r0, PCG's bi_prod and the relative residual of
   //            one solve share one reduction and one read-back
   unsigned long long   version = 1, zero_at = 0, bb_at = 0;
   double               bb = 0.0;
   void                 touch() { version++; }
   void                 mark_zero() { zero_at = version; }
   bool                 known_zero() const { return zero_at == version && stage.empty() && nloc > 0; }
   double              *data() { touch(); return view ? view : d.data(); }
   const double        *cdata() const { return view ? view : d.data(); }
   void                 ensure_device();
};
namespace hda {
bool   known_zero_enabled();                        // HDA_KNOWN_ZERO (default on), read per call
double vector_self_dot(hypre_IJVector_struct *v);   // <v,v>: cached per (vector, version) when the switch is on
} // namespace hda

namespace hda {
// device-side stack of the (local row, global column, value, set / add) entries that HYPRE_IJMatrixSetValues / AddToValues were handed
// through device pointers, in call order; grows by doubling
struct IjStack {
   DArray<int>           row;
   DArray<long long>     col;
   DArray<double>        val;
   DArray<unsigned char> add;
   size_t                size = 0;
   void                  reserve(size_t need); // room for `need` entries, the first `size` kept
   void                  clear();
};
} // namespace hda

struct hypre_IJMatrix_struct {
   MPI_Comm  comm = MPI_COMM_WORLD;
   long long ilower = 0, iupper = -1, jlower = 0, jupper = -1;
   int       nloc = 0;
   bool      initialized = false, assembled = false;
   // host staging (HYPRE_IJMatrixSetValues / AddToValues before Assemble)
   std::vector<int>       t_row;
   std::vector<long long> t_col;
   std::vector<double>    t_val;
   std::vector<char>      t_add;
   // what the last Initialize_v2 was given: where the caller's rows / cols / values arrays live.  DEVICE: the calls stack up in HBM
   HYPRE_MemoryLocation   location = HYPRE_MEMORY_HOST;
   hda::IjStack           stack;
   // assembled, HBM resident
   hda::DCsr              A;          // columns: [0,nloc) owned, >= nloc ghosts
   std::vector<long long> ghost_gids; // ascending global ids of the ghost columns
   std::vector<long long> part;       // row starts of every rank (size+1)
   hda::HaloPlan          halo;
   long long              global_rows = 0, global_nnz = 0;
   void                   assemble();
   // adopt a block that was built directly in HBM with global column ids (generator path)
   // (refuse_duplicates: returns false -- nothing adopted -- when a row names a column twice; the caller then stages triplets instead)
   bool adopt_device(int nloc, int nnz, hda::DArray<int> &rowptr, hda::DArray<long long> &gcols, hda::DArray<double> &vals,
                     bool refuse_duplicates = false);
   // a host CSR block with global column ids (HYPREDRV_LinearSystemSetMatrixFromCSR): uploaded as it is, columns mapped, rows sorted
   // and checked on the device; false = a row has a duplicate column (the staged path defines what that means)
   bool assemble_csr(const long long *indptr, const long long *cols, const double *data);
   // the same for a block that is in HBM already: indptr (nloc + 1, any base), gcols / vals its nnz entries.  vals is adopted
   bool assemble_csr_device(hda::DArray<long long> &indptr, hda::DArray<long long> &gcols, hda::DArray<double> &vals, long long nnz);
   // pieces of the two above that the device IJ path (hda_ij_device.hip) shares: ghost_gids from nnz global columns in HBM; their local
   // numbers (owned: c - jlower, ghosts: behind them in ghost_gids order); partition, halo plan and the assembled mark for a finished A
   void collect_ghosts(const long long *gcols, long long nnz);
   void map_columns(const long long *gcols, long long nnz, int *out) const;
   void finish_assembly();
   void assemble_device(); // from `stack`: bit for bit what assemble() builds from the same calls
};
namespace hda {
// what the last assemble_device() of this rank did (test / measurement entry hda_ij_last_assembly): path 0 nothing stacked, 1 the
// stack was a CSR block, 2 sort and run reduction; entries stacked and merged; stream time of the sort and of the run-reduce kernel
struct IjAssemblyStats {
   int       path = 0;
   long long stacked = 0, merged = 0;
   double    sort_ms = 0.0, reduce_ms = 0.0;
};
IjAssemblyStats &ij_assembly_stats();
// HYPRE_IJMatrixSetValues / AddToValues with device pointers: false = a row outside the local range (the rows before it are stacked,
// as the host path stacks them)
bool ij_matrix_push_device(hypre_IJMatrix_struct *m, int nrows, const int *ncols, const long long *rows, const long long *cols,
                           const double *vals, bool add);
// HYPRE_IJVectorSetValues / AddToValues / GetValues with device pointers (idx may be NULL): false = an index outside the local range
// (the entries before it are applied / returned)
bool ij_vector_set_device(hypre_IJVector_struct *v, int n, const long long *idx, const double *val, bool add);
bool ij_vector_get_device(hypre_IJVector_struct *v, int n, const long long *idx, double *out);
} // namespace hda

enum hda_solver_kind { HDA_SOLVER_PCG = 1, HDA_SOLVER_GMRES = 2, HDA_SOLVER_AMG = 3, HDA_SOLVER_ILU = 4, HDA_SOLVER_FGMRES = 5, HDA_SOLVER_BICGSTAB = 6, HDA_SOLVER_MGR = 7, HDA_SOLVER_SCHWARZ = 8, HDA_SOLVER_AMS = 9, HDA_SOLVER_FSAI = 10 };

namespace hda {
// addresses of the live solver objects THIS library created: an opaque HYPRE_Solver a caller installs with
// HYPRE_PCGSetPrecond (hypredrive's cookie, a user's own struct) may only be looked into when it is one of them
void solver_registry(const void *p, int op); // op: +1 insert, -1 erase
bool is_live_solver(const void *p);
} // namespace hda

struct hypre_Solver_struct {
   hypre_Solver_struct() { hda::solver_registry(this, +1); }
   ~hypre_Solver_struct() { hda::solver_registry(this, -1); }
   hypre_Solver_struct(const hypre_Solver_struct &) = delete;
   hypre_Solver_struct &operator=(const hypre_Solver_struct &) = delete;
   int                       kind = 0;
   hda::KrylovParams         kp;
   hda::AmgParams            ap;
   // values of setters whose feature is not implemented (checked at Setup)
   const int                *dof_func_ptr = nullptr; // HYPRE_BoomerAMGSetDofFunc (borrowed until Setup)
   double                    agg_trunc[4] = {0.0, 0.0, 0.0, 0.0}; // AggTruncFactor, AggP12TruncFactor, AggPMaxElmts, AggP12MaxElmts: [0] / [2] truncate the aggressive levels' interpolation (multipass rows, second stage of types 5 / 6); the P12 pair truncates the first stage of the two-stage types 5 / 6
   int                       smooth_type = 5, smooth_num_levels = 0, agg_num_levels = 0, num_functions = 1, cycle_type = 1,
                             restriction = 0, relax_order = 0, sabs = 0, seq_threshold = 0, relax_type_all = -1, filter_functions = 0;
   HYPRE_PtrToSolverFcn      precond = nullptr, precond_setup = nullptr;
   HYPRE_Solver              precond_solver = nullptr;
   hda::Precond              pc; // what Setup built: the object of this handle's kind, with the work vectors of its solves
   // HYPRE_BoomerAMGSetGridRelaxPoints: a copy of the schedule (down, up, coarse; one entry per sweep as the sweep counts were when it
   // was set), checked at Setup
   bool                      grid_points_set = false;
   std::vector<int>          grid_points[3];
   // HYPRE_ILU* handle, and the ILU arguments of BoomerAMG's complex smoother (HYPRE_BoomerAMGSetILU*)
   hda::IluParams            ilup;
   int                       ilu_type = 0, ilu_fill = 0, ilu_reordering = 0; // checked at Setup: bj-iluk / 0 / 0 only
   // HYPRE_Schwarz* handle: what the setters recorded (hypre's numbering: variant 10 ras-iluk, 11 as-iluk, ...), checked at Setup
   int                           sw_variant = 0, sw_overlap = 1, sw_domain_type = 2, sw_num_functions = 1, sw_nonsymm = 0, sw_local_solver = 0,
                                 sw_fill = 0, sw_max_iter = 1, sw_print_level = 0, sw_logging = 0;
   double                        sw_weight = 1.0, sw_tol = 0.0;
   // HYPRE_FSAI* handle, and the FSAI arguments of BoomerAMG's complex smoother (HYPRE_BoomerAMGSetFSAI*): what the setters recorded
   // (defaults: the reference's, src/internal/fsai.c:15-27 -- algo_type 1, the adaptive bj-afsai), checked at Setup
   hda::FsaiParams               fsaip;
   int                           fs_algo = 1, fs_ls_type = 1, fs_max_steps = 5, fs_max_step_size = 3, fs_print_level = 0;
   double                        fs_kap_tol = 1.0e-3, fs_tol = 0.0;
   // HYPRE_AMS* handle: what the setters recorded (defaults: the reference's GPU build, src/internal/ams.c:15-22), checked at Setup; G and
   // the coordinate vectors are borrowed, as in hypre
   hda::AmsParams                amsp;
   hda::AmsAmgOptions            ams_alpha, ams_beta;
   int                           ams_print_level = 0, ams_proj_freq = 5; // (proj_freq and omega act in the singular case / with relax_type 2 only)
   double                        ams_omega = 1.0;
   HYPRE_ParCSRMatrix            ams_G = nullptr;
   HYPRE_ParVector               ams_xyz[3] = {nullptr, nullptr, nullptr};
   // HYPRE_MGR* handle: what the setters recorded (hypre's per-level arrays, copied), built at Setup
   int                           mgr_block_size = 0, mgr_levels = 0, mgr_max_iter = 1, mgr_cycle = 1, mgr_frelax_cycle = 1, mgr_gsmooth_cycle = 1;
   double                        mgr_coarse_th = 0.0;
   int                           mgr_nonglk_max_elmts = 1; // HYPRE_MGRSetNonGalerkinMaxElmts (hypre's default 1)
   std::vector<std::vector<int>> mgr_c_labels; // C labels of every reduction level
   const HYPRE_Int              *mgr_marker = nullptr; // borrowed until Setup, as in hypre
   std::vector<int>              mgr_frelax, mgr_fsweeps, mgr_interp, mgr_restrict, mgr_coarse_method, mgr_gsmooth, mgr_giters;
   HYPRE_Solver                  mgr_csolver = nullptr;
   std::vector<HYPRE_Solver>     mgr_fsolver, mgr_gsolver; // F-relaxation / global smoother handles by level (HYPRE_MGRSetFSolverAtLevel / SetGlobalSmootherAtLevel)
   hda::KrylovResult         last;
   int                       amg_iters = 0;
   double                    amg_rel   = 0.0;
};

namespace hda {
// what a HYPREDRV object holds (defined in hda_hypredrv.hip): level-0 operator, its halo plan, device rhs, hierarchy
bool hypredrv_peek(void *hypredrv, const DCsr **A, const HaloPlan **halo, const double **rhs, Amg **amg);
// Schwarz selections (hypre's numbers, reference src/internal/schwarz.c:48-66): the reason why this one is not built, empty = built
std::string schwarz_refusal(int variant, int local_solver, int overlap, int fill, int max_iter, double tol, int num_functions,
                            int domain_type, int nonsymm);
// FSAI selections (reference src/internal/fsai.c:45: algo_type 1 bj-afsai, 2 bj-afsai-omp, 3 bj-sfsai): the reason why this one is not
// built, by the name of its key; empty = built
std::string fsai_refusal(int algo_type, const FsaiParams &p, double tol);
// error text of the last failed HYPRE_* call (HYPRE_GetError returns the code)
const std::string &hypre_last_error();
int                hypre_set_error(int code, const std::string &msg);
// hints the Krylov loops pass to HYPRE_BoomerAMGSolve through the C callback seam
struct PrecondHints {
   bool zero_guess = false; // the output vector is known to be zero
   int  dot_slot   = -1;    // fuse block partials of <b, x> into the last sweep
   bool dot_done   = false; // set by the callee when it honoured dot_slot
};
PrecondHints &precond_hints();
} // namespace hda
