// hda_hypre.hip -- HYPRE_* subset (include/HYPRE.h) over HBM-resident objects.
// This is the lower seam of the drop-in boundary: the functions hypredrive's op tables
// (src/internal/solver.c:204-253, src/internal/precon.c:106-157 in the reference) bind.
#include "hda_hypre.h"
#include "hda_mpi_join.h"

#include <unordered_set>

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace hda;

#define STREAM (Context::get().stream)

namespace hda {
#define g_herr (RankState<std::string, 2>::get())
#define g_hcode (RankState<int, 2>::get())
const std::string &hypre_last_error() { return g_herr; }
int hypre_set_error(int code, const std::string &msg)
{
   g_hcode |= code;
   g_herr = msg;
   return code;
}
PrecondHints &precond_hints()
{
   PrecondHints &h = RankState<PrecondHints>::get();
   return h;
}
} // namespace hda

#define HY_TRY try {
#define HY_CATCH                                                  \
   }                                                              \
   catch (const std::exception &e) { return hypre_set_error(HYPRE_ERROR_GENERIC, e.what()); } \
   return 0;

static bool have_device()
{
   int n = 0;
   return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}
#define HY_NEED_DEVICE \
   if (!have_device()) return hypre_set_error(HYPRE_ERROR_GENERIC, "no HIP device visible: the MI355X solve path has no CPU fallback")
// HDA_BLOCKS = V row blocks on one GPU (0: the setup's own choice); unset: dflt
static int  env_blocks(int dflt) { const char *e = getenv("HDA_BLOCKS"); return e ? std::max(atoi(e), 0) : dflt; }
static bool quiet() { return getenv("HDA_QUIET") != nullptr; } // HDA_QUIET: no notes about row blocks on stderr

// ------------------------------------------------------------------ utilities

extern "C" HYPRE_Int HYPRE_Initialize(void) { return 0; }
extern "C" HYPRE_Int HYPRE_Finalize(void)
{
   mpi_leave(); // lower-seam callers (an unmodified libHYPREDRV on top of this library) end here, before MPI_Finalize
   return 0;
}
extern "C" HYPRE_Int HYPRE_SetMemoryLocation(HYPRE_MemoryLocation) { return 0; }
extern "C" HYPRE_Int HYPRE_SetExecutionPolicy(HYPRE_ExecutionPolicy) { return 0; }
extern "C" HYPRE_Int HYPRE_GetError(void) { return g_hcode; }
extern "C" HYPRE_Int HYPRE_ClearAllErrors(void)
{
   g_hcode = 0;
   g_herr.clear();
   return 0;
}
extern "C" HYPRE_Int HYPRE_CheckError(HYPRE_Int ierr, HYPRE_Int code) { return ierr & code; }
// hypre's contract: descr has room for 128 characters.  The text of the last failed call of this rank when there is one (it names
// what was refused), else the meaning of the bits of ierr
extern "C" HYPRE_Int HYPRE_DescribeError(HYPRE_Int ierr, char *descr)
{
   if (!descr) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_DescribeError: null buffer");
   std::string t = g_herr;
   if (t.empty())
      t = !ierr ? "[No error] " : std::string(ierr & HYPRE_ERROR_GENERIC ? "[Generic error] " : "") + (ierr & HYPRE_ERROR_MEMORY ? "[Memory error] " : "") +
                                     (ierr & HYPRE_ERROR_ARG ? "[Error in argument] " : "") + (ierr & HYPRE_ERROR_CONV ? "[Method did not converge] " : "");
   snprintf(descr, 128, "%s", t.c_str());
   return 0;
}

// --------------------------------------------------------------------- vectors

void hypre_IJVector_struct::ensure_device()
{
   if (view) return;
   if (d.size() < (size_t)std::max(nloc, 1))
   {
      d.alloc((size_t)std::max(nloc, 1));
      d.zero();
      capacity = d.size();
      touch();
   }
}

namespace hda {
bool known_zero_enabled()
{
   // One rank only: the counters are per rank, and a rank that skips a reduction or a halo refresh its neighbours still run
   // would leave them waiting (a caller may well set values on one rank's rows alone).
   if (Comm::world().size > 1) return false;
   const char *e = getenv("HDA_KNOWN_ZERO"); // (read per call: the tests switch it inside one process)
   return !(e && atoi(e) == 0);
}
double vector_self_dot(hypre_IJVector_struct *v)
{
   const bool cache = known_zero_enabled();
   if (cache && v->bb_at == v->version) return v->bb;
   dot(v->nloc, v->cdata(), v->cdata(), 0);
   finalize(0, S_TMP);
   const double bb = read_scalar(S_TMP);
   if (cache)
   {
      v->bb    = bb;
      v->bb_at = v->version;
   }
   return bb;
}
} // namespace hda

extern "C" HYPRE_Int HYPRE_IJVectorCreate(MPI_Comm comm, HYPRE_BigInt jlower, HYPRE_BigInt jupper, HYPRE_IJVector *vector)
{
   HY_TRY
   mpi_autojoin((int)comm); // lower-seam callers hand their communicator over here (hda_mpi.cpp)
   auto *v   = new hypre_IJVector_struct();
   v->comm   = comm;
   v->jlower = jlower;
   v->jupper = jupper;
   v->nloc   = (int)std::max<long long>(jupper - jlower + 1, 0);
   *vector   = v;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJVectorDestroy(HYPRE_IJVector v)
{
   if (v)
   {
      try { if (have_device()) Context::get().sync(); } catch (...) {}
      delete v;
   }
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJVectorSetObjectType(HYPRE_IJVector, HYPRE_Int) { return 0; }
extern "C" HYPRE_Int HYPRE_IJVectorInitialize_v2(HYPRE_IJVector v, HYPRE_MemoryLocation loc)
{
   HY_TRY
   v->location = loc == HYPRE_MEMORY_DEVICE ? HYPRE_MEMORY_DEVICE : HYPRE_MEMORY_HOST;
   if (v->location == HYPRE_MEMORY_DEVICE)
   { // the values live in HBM from the start: zero there (on a machine without a device the first Set / Get call is the one refused)
      std::vector<double>().swap(v->stage);
      if (have_device())
      {
         v->ensure_device();
         if (v->nloc) HDA_HIP(hipMemsetAsync(v->data(), 0, sizeof(double) * (size_t)v->nloc, STREAM));
      }
   }
   else v->stage.assign((size_t)v->nloc, 0.0);
   v->touch();
   v->initialized = true;
   v->assembled   = false;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJVectorInitialize(HYPRE_IJVector v) { return HYPRE_IJVectorInitialize_v2(v, HYPRE_MEMORY_HOST); }

static HYPRE_Int vec_set(HYPRE_IJVector v, HYPRE_Int n, const HYPRE_BigInt *idx, const HYPRE_Complex *val, bool add)
{
   if (v->location == HYPRE_MEMORY_DEVICE)
   { // idx (or NULL) and val are device pointers: applied to the HBM storage at once, in call order (hda_ij_device.hip)
      HY_NEED_DEVICE;
      HY_TRY
      const bool ok = ij_vector_set_device(v, n, idx, val, add);
      v->assembled  = false;
      if (!ok) return hypre_set_error(HYPRE_ERROR_ARG, "IJVector index outside the local range");
      HY_CATCH
   }
   HY_TRY
   if (!v->initialized) HYPRE_IJVectorInitialize(v);
   if (v->assembled && v->stage.empty())
   { // re-open an assembled vector: pull the device values back into the stage
      v->stage.resize((size_t)v->nloc);
      download_sync(v->stage.data(), v->cdata(), sizeof(double) * (size_t)v->nloc);
   }
   v->touch();
   for (int q = 0; q < n; q++)
   {
      const long long l = idx ? idx[q] - v->jlower : q;
      if (l < 0 || l >= v->nloc) return hypre_set_error(HYPRE_ERROR_ARG, "IJVector index outside the local range");
      if (add) v->stage[(size_t)l] += val[q];
      else v->stage[(size_t)l] = val[q];
   }
   v->assembled = false;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJVectorSetValues(HYPRE_IJVector v, HYPRE_Int n, const HYPRE_BigInt *idx, const HYPRE_Complex *val)
{
   return vec_set(v, n, idx, val, false);
}
extern "C" HYPRE_Int HYPRE_IJVectorAddToValues(HYPRE_IJVector v, HYPRE_Int n, const HYPRE_BigInt *idx, const HYPRE_Complex *val)
{
   return vec_set(v, n, idx, val, true);
}
extern "C" HYPRE_Int HYPRE_IJVectorAssemble(HYPRE_IJVector v)
{
   HY_NEED_DEVICE;
   HY_TRY
   v->touch();
   if (!v->stage.empty() || v->nloc == 0)
   {
      v->d.alloc((size_t)std::max(v->nloc, 1));
      v->capacity = v->d.size();
      if (v->nloc) v->d.upload(v->stage.data(), (size_t)v->nloc);
      std::vector<double>().swap(v->stage);
   }
   v->assembled = true;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJVectorGetValues(HYPRE_IJVector v, HYPRE_Int n, const HYPRE_BigInt *idx, HYPRE_Complex *val)
{
   if (v->location == HYPRE_MEMORY_DEVICE)
   { // idx (or NULL) and val are device pointers
      HY_NEED_DEVICE;
      HY_TRY
      if (!ij_vector_get_device(v, n, idx, val)) return hypre_set_error(HYPRE_ERROR_ARG, "IJVector index outside the local range");
      HY_CATCH
   }
   HY_TRY
   std::vector<double> h;
   const double       *src;
   if (!v->stage.empty()) src = v->stage.data();
   else
   {
      h.resize((size_t)std::max(v->nloc, 1));
      download_sync(h.data(), v->cdata(), sizeof(double) * (size_t)v->nloc);
      src = h.data();
   }
   for (int q = 0; q < n; q++)
   {
      const long long l = idx ? idx[q] - v->jlower : q;
      if (l < 0 || l >= v->nloc) return hypre_set_error(HYPRE_ERROR_ARG, "IJVector index outside the local range");
      val[q] = src[l];
   }
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJVectorGetObject(HYPRE_IJVector v, void **object)
{
   *object = v;
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJVectorGetLocalRange(HYPRE_IJVector v, HYPRE_BigInt *jl, HYPRE_BigInt *ju)
{
   *jl = v->jlower;
   *ju = v->jupper;
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJVectorMigrate(HYPRE_IJVector v, HYPRE_MemoryLocation) { return v->assembled ? 0 : HYPRE_IJVectorAssemble(v); }

static std::string rank_file(const char *prefix, int rank)
{
   char buf[32];
   snprintf(buf, sizeof(buf), ".%05d", rank);
   return std::string(prefix) + buf;
}

// Part files "<prefix>.%05d" present on disk, counted from 0 (reference src/internal/utils.c hypredrv_CountNumberOfPartitions)
static int count_part_files(const char *prefix)
{
   int n = 0;
   for (;; n++)
   {
      FILE *f = fopen(rank_file(prefix, n).c_str(), "r");
      if (!f) break;
      fclose(f);
   }
   return n;
}
static void my_parts(long long g_nparts, int &first, int &count);

// hypre ASCII IJ vector file: "jlower jupper" then "j value" lines.  With more part files than ranks
// (the np4 data set of examples/ex8.yml on one rank) a rank reads its contiguous group of parts, as the multipart binary
// reader does (reference src/internal/linsys.c:872-903 takes that route whenever parts >= ranks).
extern "C" HYPRE_Int HYPRE_IJVectorRead(const char *filename, MPI_Comm comm, HYPRE_Int, HYPRE_IJVector *vector)
{
   HY_TRY
   mpi_autojoin((int)comm);
   const int nparts = count_part_files(filename);
   int       first = Comm::world().rank, count = 1;
   if (nparts > Comm::world().size) my_parts(nparts, first, count);
   std::vector<std::pair<long long, double>> ent;
   long long lo = 0, hi = -1;
   for (int p = first; p < first + count; p++)
   {
      const std::string fn = rank_file(filename, p);
      FILE             *f  = fopen(fn.c_str(), "r");
      if (!f) return hypre_set_error(HYPRE_ERROR_ARG, "cannot open " + fn);
      long long jl, ju;
      if (fscanf(f, "%lld %lld", &jl, &ju) != 2) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "bad IJ vector header in " + fn); }
      if (p == first) lo = jl;
      else if (jl != hi + 1) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "IJ vector parts are not contiguous at " + fn); }
      hi = ju;
      long long j;
      double    val;
      while (fscanf(f, "%lld %lf", &j, &val) == 2)
      {
         if (j < jl || j > ju) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "IJ vector entry outside its header range in " + fn); }
         ent.emplace_back(j, val);
      }
      fclose(f);
   }
   HYPRE_IJVectorCreate(comm, lo, hi, vector);
   HYPRE_IJVectorInitialize(*vector);
   for (auto &e : ent) (*vector)->stage[(size_t)(e.first - lo)] = e.second;
   (*vector)->touch();
   return HYPRE_IJVectorAssemble(*vector);
   HY_CATCH
}
// hypredrive's multipart binary files (reference src/internal/vector.c:92-380, matrix.c:142-860):
// "<prefix>.<part %05d>.bin"; g_nparts parts are dealt to the ranks in contiguous groups, the
// first (g_nparts mod ranks) ranks holding one more.
static void my_parts(long long g_nparts, int &first, int &count)
{
   Comm &cm = Comm::world();
   count    = (int)(g_nparts / cm.size) + (cm.rank < (int)(g_nparts % cm.size) ? 1 : 0);
   first    = cm.rank * (int)(g_nparts / cm.size) + std::min<int>(cm.rank, (int)(g_nparts % cm.size));
}
static std::string part_file(const char *prefix, int part)
{
   char buf[40];
   snprintf(buf, sizeof(buf), ".%05d.bin", part);
   return std::string(prefix) + buf;
}
extern "C" int hda_count_binary_parts(const char *prefix)
{
   int n = 0;
   for (;; n++)
   {
      FILE *f = fopen(part_file(prefix, n).c_str(), "rb");
      if (!f) break;
      fclose(f);
   }
   return n;
}
// all ranks agree on success before anything collective happens (as the reference does)
static bool all_ok(bool mine)
{
   long long v = mine ? 0 : 1;
   Comm::world().allreduce_host(&v, 1, 1);
   return v == 0;
}

// vector part: 8 x u64 header ([1] bytes per value, [5] rows of the part), then the values
extern "C" HYPRE_Int hda_IJVectorReadMultipartBinary(const char *prefix, MPI_Comm comm, long long g_nparts, HYPRE_IJVector *vector)
{
   HY_TRY
   mpi_autojoin((int)comm);
   *vector = nullptr;
   Comm &cm = Comm::world();
   if (g_nparts < cm.size) return hypre_set_error(HYPRE_ERROR_GENERIC, "Invalid number of parts!");
   int first = 0, count = 0;
   my_parts(g_nparts, first, count);
   std::vector<double> vals;
   std::string         why;
   for (int p = first; p < first + count && why.empty(); p++)
   {
      const std::string fn = part_file(prefix, p);
      FILE             *f  = fopen(fn.c_str(), "rb");
      if (!f) { why = "cannot open " + fn; break; }
      uint64_t hd[8];
      if (fread(hd, 8, 8, f) != 8) why = "Could not read header from " + fn;
      else if (hd[5] > (1ull << 31)) why = "Vector row count exceeds per-part limit in " + fn;
      else if (hd[1] == 8)
      {
         const size_t o = vals.size();
         vals.resize(o + (size_t)hd[5]);
         if (hd[5] && fread(vals.data() + o, 8, (size_t)hd[5], f) != hd[5]) why = "Could not read coeficients from " + fn;
      }
      else if (hd[1] == 4)
      {
         std::vector<float> b((size_t)hd[5]);
         if (hd[5] && fread(b.data(), 4, (size_t)hd[5], f) != hd[5]) why = "Could not read coeficients from " + fn;
         vals.insert(vals.end(), b.begin(), b.end());
      }
      else why = "Invalid coefficient data type size at " + fn;
      fclose(f);
   }
   for (double x : vals)
      if (!std::isfinite(x) && why.empty()) why = std::string("Detected non-finite vector coefficient while reading ") + prefix;
   if (!all_ok(why.empty())) return hypre_set_error(HYPRE_ERROR_GENERIC, why.empty() ? "another rank could not read its vector parts" : why);
   std::vector<long long> cnts;
   cm.allgather_ll((long long)vals.size(), cnts);
   long long lo = 0;
   for (int r = 0; r < cm.rank; r++) lo += cnts[(size_t)r];
   HYPRE_IJVectorCreate(comm, lo, lo + (long long)vals.size() - 1, vector);
   HYPRE_IJVectorInitialize(*vector);
   std::copy(vals.begin(), vals.end(), (*vector)->stage.begin());
   (*vector)->touch();
   return HYPRE_IJVectorAssemble(*vector);
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_IJVectorPrint(HYPRE_IJVector v, const char *filename)
{
   HY_TRY
   const std::string fn = rank_file(filename, Comm::world().rank);
   FILE             *f  = fopen(fn.c_str(), "w");
   if (!f) return hypre_set_error(HYPRE_ERROR_ARG, "cannot write " + fn);
   std::vector<double> h((size_t)std::max(v->nloc, 1));
   download_sync(h.data(), v->data(), sizeof(double) * (size_t)v->nloc);
   fprintf(f, "%lld %lld\n", v->jlower, v->jupper);
   for (int i = 0; i < v->nloc; i++) fprintf(f, "%lld %.14e\n", v->jlower + i, h[(size_t)i]);
   fclose(f);
   HY_CATCH
}

// -------------------------------------------------------------------- matrices

extern "C" HYPRE_Int HYPRE_IJMatrixCreate(MPI_Comm comm, HYPRE_BigInt ilower, HYPRE_BigInt iupper, HYPRE_BigInt jlower,
                                          HYPRE_BigInt jupper, HYPRE_IJMatrix *matrix)
{
   HY_TRY
   mpi_autojoin((int)comm);
   auto *m   = new hypre_IJMatrix_struct();
   m->comm   = comm;
   m->ilower = ilower; m->iupper = iupper; m->jlower = jlower; m->jupper = jupper;
   m->nloc   = (int)std::max<long long>(iupper - ilower + 1, 0);
   *matrix   = m;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJMatrixDestroy(HYPRE_IJMatrix m)
{
   if (m)
   {
      try { if (have_device()) Context::get().sync(); } catch (...) {}
      delete m;
   }
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJMatrixSetObjectType(HYPRE_IJMatrix, HYPRE_Int) { return 0; }
extern "C" HYPRE_Int HYPRE_IJMatrixSetRowSizes(HYPRE_IJMatrix m, const HYPRE_Int *sizes)
{
   HY_TRY
   size_t tot = 0;
   for (int i = 0; i < m->nloc; i++) tot += (size_t)std::max(sizes[i], 0);
   m->t_row.reserve(tot); m->t_col.reserve(tot); m->t_val.reserve(tot); m->t_add.reserve(tot);
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJMatrixSetDiagOffdSizes(HYPRE_IJMatrix, const HYPRE_Int *, const HYPRE_Int *) { return 0; }
extern "C" HYPRE_Int HYPRE_IJMatrixInitialize_v2(HYPRE_IJMatrix m, HYPRE_MemoryLocation loc)
{
   m->location    = loc == HYPRE_MEMORY_DEVICE ? HYPRE_MEMORY_DEVICE : HYPRE_MEMORY_HOST;
   m->initialized = true;
   m->assembled   = false;
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJMatrixInitialize(HYPRE_IJMatrix m) { return HYPRE_IJMatrixInitialize_v2(m, HYPRE_MEMORY_HOST); }

static HYPRE_Int mat_set(HYPRE_IJMatrix m, HYPRE_Int nrows, HYPRE_Int *ncols, const HYPRE_BigInt *rows,
                         const HYPRE_BigInt *cols, const HYPRE_Complex *values, bool add)
{
   if (m->location == HYPRE_MEMORY_DEVICE)
   { // all four arrays are device pointers: the call goes onto the device-side stack (hda_ij_device.hip)
      HY_NEED_DEVICE;
      HY_TRY
      const bool ok = ij_matrix_push_device(m, nrows, ncols, rows, cols, values, add);
      if (!ok) return hypre_set_error(HYPRE_ERROR_ARG, "IJMatrix row outside the local range (off-rank assembly is not supported)");
      if (nrows > 0) m->assembled = false;
      HY_CATCH
   }
   HY_TRY
   size_t q = 0;
   for (int r = 0; r < nrows; r++)
   {
      const long long l = rows[r] - m->ilower;
      if (l < 0 || l >= m->nloc) return hypre_set_error(HYPRE_ERROR_ARG, "IJMatrix row outside the local range (off-rank assembly is not supported)");
      for (int c = 0; c < ncols[r]; c++, q++)
      {
         m->t_row.push_back((int)l);
         m->t_col.push_back(cols[q]);
         m->t_val.push_back(values[q]);
         m->t_add.push_back(add ? 1 : 0);
      }
   }
   m->assembled = false;
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJMatrixSetValues(HYPRE_IJMatrix m, HYPRE_Int nrows, HYPRE_Int *ncols, const HYPRE_BigInt *rows,
                                             const HYPRE_BigInt *cols, const HYPRE_Complex *values)
{
   return mat_set(m, nrows, ncols, rows, cols, values, false);
}
extern "C" HYPRE_Int HYPRE_IJMatrixAddToValues(HYPRE_IJMatrix m, HYPRE_Int nrows, HYPRE_Int *ncols, const HYPRE_BigInt *rows,
                                               const HYPRE_BigInt *cols, const HYPRE_Complex *values)
{
   return mat_set(m, nrows, ncols, rows, cols, values, true);
}

__global__ __launch_bounds__(256) void k_map_gcols(long nnz, const long long *__restrict__ gc, long long jlo, long long jhi,
                                                   int ncol_loc, const long long *__restrict__ ghosts, int nghost,
                                                   int *__restrict__ out)
{
   for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (long)gridDim.x * 256)
   {
      const long long c = gc[k];
      if (c >= jlo && c <= jhi) out[k] = (int)(c - jlo);
      else
      { // binary search in the ascending ghost list
         int lo = 0, hi = nghost - 1;
         while (lo < hi)
         {
            const int mid = (lo + hi) >> 1;
            if (ghosts[mid] < c) lo = mid + 1;
            else hi = mid;
         }
         out[k] = ncol_loc + lo;
      }
   }
}

static void finish_partition(hypre_IJMatrix_struct *m)
{
   Comm &cm = Comm::world();
   std::vector<long long> lows;
   cm.allgather_ll(m->ilower, lows);
   long long tot[2] = {m->nloc, m->A.nnz};
   cm.allreduce_host(tot, 2, 0);
   m->global_rows = tot[0];
   m->global_nnz  = tot[1];
   m->part        = lows;
   m->part.push_back(lows[0] + m->global_rows);
   for (int r = 0; r < cm.size; r++)
      HDA_REQUIRE(m->part[(size_t)r] <= m->part[(size_t)r + 1], "row ranges must ascend with the rank");
   m->halo = make_halo_plan(m->nloc, m->part, m->ghost_gids);
}

void hypre_IJMatrix_struct::assemble()
{
   const size_t T = t_row.size();
   // Rows handed over in order with plain "set" semantics (every row-at-a-time driver: reference examples/src/C_laplacian/laplacian.c:
   // 734-914) are a CSR block already: count the rows, upload the staged columns and values as they are and let the device map, sort
   // and check them (assemble_csr); a block with a column named twice in a row comes back and takes the general path below.
   if (T > 0 && T < (1ULL << 31) && !(getenv("HDA_CSR_DIRECT") && atoi(getenv("HDA_CSR_DIRECT")) == 0))
   {
      bool ordered = true;
      for (size_t q = 1; q < T && ordered; q++) ordered = t_row[q] >= t_row[q - 1];
      for (size_t q = 0; q < T && ordered; q++) ordered = !t_add[q];
      if (ordered)
      {
         std::vector<long long> ip((size_t)nloc + 1, 0);
         for (size_t q = 0; q < T; q++) ip[(size_t)t_row[q] + 1]++;
         for (int i = 0; i < nloc; i++) ip[(size_t)i + 1] += ip[(size_t)i];
         if (assemble_csr(ip.data(), t_col.data(), t_val.data()))
         {
            std::vector<int>().swap(t_row);
            std::vector<long long>().swap(t_col);
            std::vector<double>().swap(t_val);
            std::vector<char>().swap(t_add);
            return;
         }
      }
   }
   // stable counting sort of the triplets by row
   std::vector<int> rp((size_t)nloc + 1, 0);
   for (size_t q = 0; q < T; q++) rp[(size_t)t_row[q] + 1]++;
   for (int i = 0; i < nloc; i++) rp[(size_t)i + 1] += rp[(size_t)i];
   std::vector<long long> cj(std::max<size_t>(T, 1));
   std::vector<double>    cv(std::max<size_t>(T, 1));
   std::vector<char>      ca(std::max<size_t>(T, 1));
   {
      std::vector<int> pos(rp.begin(), rp.end() - 1);
      for (size_t q = 0; q < T; q++)
      {
         const int p  = pos[(size_t)t_row[q]]++;
         cj[(size_t)p] = t_col[q];
         cv[(size_t)p] = t_val[q];
         ca[(size_t)p] = t_add[q];
      }
   }
   std::vector<int>().swap(t_row);
   std::vector<long long>().swap(t_col);
   std::vector<double>().swap(t_val);
   std::vector<char>().swap(t_add);
   // merge duplicates inside each row (set: last wins, add: accumulate), keep first position
   std::vector<int> rp2((size_t)nloc + 1, 0);
   size_t           w = 0;
   for (int i = 0; i < nloc; i++)
   {
      const size_t s = (size_t)rp[(size_t)i], e = (size_t)rp[(size_t)i + 1], w0 = w;
      for (size_t q = s; q < e; q++)
      {
         size_t hit = w;
         for (size_t z = w0; z < w; z++)
            if (cj[z] == cj[q]) { hit = z; break; }
         if (hit == w) { cj[w] = cj[q]; cv[w] = cv[q]; w++; }
         else if (ca[q]) cv[hit] += cv[q];
         else cv[hit] = cv[q];
      }
      rp2[(size_t)i + 1] = (int)w;
   }
   const size_t nnz = w;
   HDA_REQUIRE(nnz < (1ULL << 31), "local nnz must fit int32");
   // ghost columns
   std::vector<long long> gh;
   for (size_t q = 0; q < nnz; q++)
      if (cj[q] < jlower || cj[q] > jupper) gh.push_back(cj[q]);
   std::sort(gh.begin(), gh.end());
   gh.erase(std::unique(gh.begin(), gh.end()), gh.end());
   ghost_gids = gh;
   DArray<int>       drp;
   DArray<long long> dgc;
   DArray<double>    dv;
   drp.upload(rp2.data(), (size_t)nloc + 1);
   dgc.upload(cj.data(), std::max<size_t>(nnz, 1));
   dv.upload(cv.data(), std::max<size_t>(nnz, 1));
   adopt_device(nloc, (int)nnz, drp, dgc, dv);
}

// entries of a block whose global column lies outside [jlo, jhi]: counted, and (second launch) written side by side
__global__ __launch_bounds__(256) void k_ghost_cols(long nnz, const long long *__restrict__ gc, long long jlo, long long jhi, unsigned long long *count,
                                                    long long *__restrict__ out)
{
   for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (long)gridDim.x * 256)
   {
      const long long c = gc[k];
      if (c < jlo || c > jhi)
      {
         const unsigned long long q = atomicAdd(count, 1ull);
         if (out) out[q] = c;
      }
   }
}
__global__ __launch_bounds__(256) void k_indptr_to_rowptr(int n, const long long *__restrict__ ip, int *__restrict__ rp)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i <= n) rp[i] = (int)(ip[i] - ip[0]);
}
__global__ __launch_bounds__(256) void k_row_has_duplicate(int n, const int *__restrict__ rp, const int *__restrict__ cj, int *flag)
{ // rows are column-sorted: a duplicate is two equal neighbours
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   for (int k = rp[i] + 1; k < rp[i + 1]; k++)
      if (cj[k] == cj[k - 1]) { *flag = 1; return; }
}

bool hypre_IJMatrix_struct::assemble_csr(const long long *indptr, const long long *cols, const double *data)
{
   const long long nnz = indptr[nloc] - indptr[0];
   DArray<long long> dip, dgc;
   DArray<double>    dv;
   dip.upload(indptr, (size_t)nloc + 1);
   if (nnz)
   {
      dgc.upload(cols + indptr[0], (size_t)nnz);
      dv.upload(data + indptr[0], (size_t)nnz);
   }
   else
   { // a block without entries (cols / data may be NULL: reference tests/test_setmatrix_from_csr.c:483)
      dgc.alloc(1);
      dv.alloc(1);
   }
   return assemble_csr_device(dip, dgc, dv, nnz);
}

bool hypre_IJMatrix_struct::assemble_csr_device(DArray<long long> &dip, DArray<long long> &dgc, DArray<double> &dv, long long nnz)
{
   DArray<int> drp((size_t)nloc + 1);
   k_indptr_to_rowptr<<<ceil_div(nloc + 1, 256), 256, 0, STREAM>>>(nloc, dip.data(), drp.data());
   collect_ghosts(dgc.data(), nnz);
   return adopt_device(nloc, (int)nnz, drp, dgc, dv, true);
}

// ghost columns: the few entries that leave [jlower, jupper] are collected on the device, sorted and made unique on the host
void hypre_IJMatrix_struct::collect_ghosts(const long long *gcols, long long nnz)
{
   ghost_gids.clear();
   if (!nnz) return;
   DArray<unsigned long long> cnt(1);
   cnt.zero();
   const int g = std::min(ceil_div(nnz, 256), 1 << 16);
   k_ghost_cols<<<g, 256, 0, STREAM>>>((long)nnz, gcols, jlower, jupper, cnt.data(), nullptr);
   unsigned long long ng = 0;
   cnt.download(&ng, 1);
   if (ng)
   {
      DArray<long long> out((size_t)ng);
      cnt.zero();
      k_ghost_cols<<<g, 256, 0, STREAM>>>((long)nnz, gcols, jlower, jupper, cnt.data(), out.data());
      std::vector<long long> gh = out.to_host();
      std::sort(gh.begin(), gh.end());
      gh.erase(std::unique(gh.begin(), gh.end()), gh.end());
      ghost_gids = gh;
   }
}

void hypre_IJMatrix_struct::map_columns(const long long *gcols, long long nnz, int *out) const
{
   if (!nnz) return;
   DArray<long long> dgh;
   if (!ghost_gids.empty()) dgh.upload(ghost_gids.data(), ghost_gids.size());
   k_map_gcols<<<std::min(ceil_div(nnz, 256), 1 << 16), 256, 0, STREAM>>>((long)nnz, gcols, jlower, jupper, (int)(jupper - jlower + 1), dgh.data(),
                                                                         (int)ghost_gids.size(), out);
}

void hypre_IJMatrix_struct::finish_assembly()
{
   Context::get().sync();
   finish_partition(this);
   assembled = true;
}

bool hypre_IJMatrix_struct::adopt_device(int nl, int nnz, DArray<int> &rowptr, DArray<long long> &gcols, DArray<double> &vals, bool refuse_duplicates)
{
   // ghost list must already be in ghost_gids (ascending); single-rank callers leave it empty
   const int ncol_loc = (int)(jupper - jlower + 1);
   A.nrows            = nl;
   A.nnz              = nnz;
   A.ncols            = ncol_loc + (int)ghost_gids.size();
   A.rowptr           = std::move(rowptr);
   A.val              = std::move(vals);
   A.col.alloc((size_t)std::max(nnz, 1));
   DArray<long long> dgh;
   if (!ghost_gids.empty()) dgh.upload(ghost_gids.data(), ghost_gids.size());
   if (nnz)
      k_map_gcols<<<std::min(ceil_div(nnz, 256), 1 << 16), 256, 0, STREAM>>>(nnz, gcols.data(), jlower, jupper, ncol_loc,
                                                                           dgh.data(), (int)ghost_gids.size(), A.col.data());
   sort_rows(A);
   if (refuse_duplicates && nnz)
   {
      DArray<int> flag(1);
      flag.zero();
      k_row_has_duplicate<<<ceil_div(nl, 256), 256, 0, STREAM>>>(nl, A.rowptr.data(), A.col.data(), flag.data());
      int f = 0;
      flag.download(&f, 1);
      if (f)
      {
         A = DCsr();
         ghost_gids.clear();
         return false;
      }
   }
   Context::get().sync();
   finish_partition(this);
   assembled = true;
   return true;
}

extern "C" HYPRE_Int HYPRE_IJMatrixAssemble(HYPRE_IJMatrix m)
{
   HY_NEED_DEVICE;
   HY_TRY
   set_stage("matrix assembly (HYPRE_IJMatrixAssemble)");
   if (m->location == HYPRE_MEMORY_DEVICE)
   { // the calls since Initialize_v2(DEVICE) are on the device-side stack
      HDA_REQUIRE(m->t_row.empty(), "an IJMatrix initialised with HYPRE_MEMORY_DEVICE still holds values set through host pointers");
      if (m->assembled && m->stack.size == 0) return 0;
      HDA_REQUIRE(!m->assembled, "re-assembly of an assembled IJMatrix with new values is not supported");
      m->assemble_device();
      return 0;
   }
   HDA_REQUIRE(m->stack.size == 0, "an IJMatrix initialised with HYPRE_MEMORY_HOST still holds values set through device pointers");
   if (m->assembled && m->t_row.empty()) return 0;
   HDA_REQUIRE(!m->assembled || m->t_row.empty(), "re-assembly of an assembled IJMatrix with new values is not supported");
   m->assemble();
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_IJMatrixGetObject(HYPRE_IJMatrix m, void **object)
{
   *object = m;
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJMatrixGetLocalRange(HYPRE_IJMatrix m, HYPRE_BigInt *il, HYPRE_BigInt *iu, HYPRE_BigInt *jl, HYPRE_BigInt *ju)
{
   *il = m->ilower; *iu = m->iupper; *jl = m->jlower; *ju = m->jupper;
   return 0;
}
extern "C" HYPRE_Int HYPRE_IJMatrixMigrate(HYPRE_IJMatrix m, HYPRE_MemoryLocation) { return m->assembled ? 0 : HYPRE_IJMatrixAssemble(m); }
extern "C" HYPRE_Int HYPRE_ParCSRMatrixGetDims(HYPRE_ParCSRMatrix A, HYPRE_BigInt *M, HYPRE_BigInt *N)
{
   if (M) *M = A->global_rows;
   if (N) *N = A->global_rows;
   return 0;
}
extern "C" HYPRE_Int HYPRE_ParCSRMatrixGetNumNonzeros(HYPRE_ParCSRMatrix A, HYPRE_BigInt *nnz)
{
   *nnz = A->global_nnz;
   return 0;
}

// hypre ASCII IJ matrix file: "ilower iupper jlower jupper" then "i j value" 
extern "C" HYPRE_Int HYPRE_IJMatrixRead(const char *filename, MPI_Comm comm, HYPRE_Int, HYPRE_IJMatrix *matrix)
{
   HY_TRY
   mpi_autojoin((int)comm);
   // more part files than ranks: a rank reads its contiguous group of parts (see HYPRE_IJVectorRead)
   const int nparts = count_part_files(filename);
   int       first = Comm::world().rank, count = 1;
   if (nparts > Comm::world().size) my_parts(nparts, first, count);
   std::vector<long long> ti, tj;
   std::vector<double>    tv;
   long long              lo = 0, hi = -1, clo = 0, chi = -1;
   for (int p = first; p < first + count; p++)
   {
      const std::string fn = rank_file(filename, p);
      FILE             *f  = fopen(fn.c_str(), "r");
      if (!f) return hypre_set_error(HYPRE_ERROR_ARG, "cannot open " + fn);
      long long il, iu, jl, ju;
      if (fscanf(f, "%lld %lld %lld %lld", &il, &iu, &jl, &ju) != 4) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "bad IJ matrix header in " + fn); }
      if (p == first) { lo = il; clo = jl; }
      else if (il != hi + 1) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "IJ matrix parts are not contiguous at " + fn); }
      hi  = iu;
      chi = ju;
      long long i, j;
      double    v;
      while (fscanf(f, "%lld %lld %lf", &i, &j, &v) == 3)
      {
         if (i < il || i > iu) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, "IJ matrix row outside its header range in " + fn); }
         ti.push_back(i);
         tj.push_back(j);
         tv.push_back(v);
      }
      fclose(f);
   }
   HYPRE_IJMatrixCreate(comm, lo, hi, clo, chi, matrix);
   HYPRE_IJMatrixInitialize(*matrix);
   auto *m = *matrix;
   m->t_row.reserve(ti.size());
   for (size_t q = 0; q < ti.size(); q++)
   {
      m->t_row.push_back((int)(ti[q] - lo));
      m->t_col.push_back(tj[q]);
      m->t_val.push_back(tv[q]);
      m->t_add.push_back(0);
   }
   return HYPRE_IJMatrixAssemble(m);
   HY_CATCH
}
// matrix part: 11 x u64 header ([1] bytes per index, [2] bytes per value, [3]/[4] global rows /
// columns, [6] entries of the part, [7]..[8] its rows), then rows[], cols[] (global ids), vals[]
extern "C" HYPRE_Int hda_IJMatrixReadMultipartBinary(const char *prefix, MPI_Comm comm, long long g_nparts, HYPRE_IJMatrix *matrix)
{
   HY_TRY
   mpi_autojoin((int)comm);
   *matrix = nullptr;
   Comm &cm = Comm::world();
   if (g_nparts < cm.size) return hypre_set_error(HYPRE_ERROR_GENERIC, "Invalid number of parts!");
   int first = 0, count = 0;
   my_parts(g_nparts, first, count);
   std::vector<long long> rows, cols;
   std::vector<double>    vals;
   long long              nrows_mine = 0;
   std::string            why;
   auto read_idx = [&](FILE *f, uint64_t width, uint64_t n, std::vector<long long> &out) -> bool {
      const size_t o = out.size();
      out.resize(o + (size_t)n);
      if (width == 8) return n == 0 || fread(out.data() + o, 8, (size_t)n, f) == n;
      std::vector<uint32_t> b((size_t)n);
      if (n && fread(b.data(), 4, (size_t)n, f) != n) return false;
      for (size_t q = 0; q < (size_t)n; q++) out[o + q] = (long long)b[q];
      return true;
   };
   for (int p = first; p < first + count && why.empty(); p++)
   {
      const std::string fn = part_file(prefix, p);
      FILE             *f  = fopen(fn.c_str(), "rb");
      if (!f) { why = "cannot open " + fn; break; }
      uint64_t hd[11];
      if (fread(hd, 8, 11, f) != 11) why = "Could not read header from " + fn;
      else if (hd[8] < hd[7]) why = "Invalid matrix row range in " + fn;
      else if (hd[1] != 4 && hd[1] != 8) why = "Invalid row/col data type size at " + fn;
      else if (hd[2] != 4 && hd[2] != 8) why = "Invalid coefficient data type size at " + fn;
      else if (hd[6] > (1ull << 31)) why = "Matrix nnz exceeds per-part limit in " + fn;
      else
      {
         const size_t o = rows.size();
         if (!read_idx(f, hd[1], hd[6], rows) || !read_idx(f, hd[1], hd[6], cols)) why = "Could not read row/column indices from " + fn;
         else if (hd[2] == 8)
         {
            vals.resize(o + (size_t)hd[6]);
            if (hd[6] && fread(vals.data() + o, 8, (size_t)hd[6], f) != hd[6]) why = "Could not read coefficients from " + fn;
         }
         else
         {
            std::vector<float> b((size_t)hd[6]);
            if (hd[6] && fread(b.data(), 4, (size_t)hd[6], f) != hd[6]) why = "Could not read coefficients from " + fn;
            vals.insert(vals.end(), b.begin(), b.end());
         }
         for (size_t q = o; q < rows.size() && why.empty(); q++)
         {
            if (rows[q] < 0 || cols[q] < 0 || (uint64_t)rows[q] >= hd[3] || (uint64_t)cols[q] >= hd[4])
               why = "Detected out-of-bounds matrix entry while reading " + fn;
            else if (q < vals.size() && !std::isfinite(vals[q])) why = "Detected non-finite matrix coefficient while reading " + fn;
         }
         nrows_mine += (long long)(hd[8] - hd[7] + 1);
      }
      fclose(f);
   }
   if (!all_ok(why.empty())) return hypre_set_error(HYPRE_ERROR_GENERIC, why.empty() ? "another rank could not read its matrix parts" : why);
   std::vector<long long> cnts;
   cm.allgather_ll(nrows_mine, cnts);
   long long lo = 0;
   for (int r = 0; r < cm.rank; r++) lo += cnts[(size_t)r];
   HYPRE_IJMatrixCreate(comm, lo, lo + nrows_mine - 1, lo, lo + nrows_mine - 1, matrix);
   HYPRE_IJMatrixInitialize(*matrix);
   auto *m = *matrix;
   for (size_t q = 0; q < rows.size(); q++)
   {
      if (rows[q] < lo || rows[q] >= lo + nrows_mine) return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("matrix part holds a row outside its rank's block in ") + prefix);
      m->t_row.push_back((int)(rows[q] - lo));
      m->t_col.push_back(cols[q]);
      m->t_val.push_back(vals[q]);
      m->t_add.push_back(0);
   }
   return HYPRE_IJMatrixAssemble(m);
   HY_CATCH
}

// Matrix Market coordinate file (real / integer / pattern; general or symmetric), one file for
// the whole matrix: every rank parses it and keeps an equal contiguous block of rows.
extern "C" HYPRE_Int HYPRE_IJMatrixReadMM(const char *filename, MPI_Comm comm, HYPRE_Int, HYPRE_IJMatrix *matrix)
{
   HY_TRY
   mpi_autojoin((int)comm);
   *matrix = nullptr;
   FILE *f = fopen(filename, "r");
   if (!f) return hypre_set_error(HYPRE_ERROR_ARG, std::string("cannot open ") + filename);
   char line[1024];
   if (!fgets(line, sizeof(line), f)) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("empty Matrix Market file ") + filename); }
   std::string banner(line);
   for (auto &c : banner) c = (char)tolower(c);
   if (banner.find("%%matrixmarket") != 0 || banner.find("coordinate") == std::string::npos || banner.find("complex") != std::string::npos)
   {
      fclose(f);
      return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("unsupported Matrix Market banner in ") + filename);
   }
   const bool pattern = banner.find("pattern") != std::string::npos;
   const bool sym     = banner.find(" symmetric") != std::string::npos;
   const bool skew    = banner.find("skew-symmetric") != std::string::npos;
   long long  M = 0, N = 0, NZ = 0;
   while (fgets(line, sizeof(line), f))
      if (line[0] != '%' && sscanf(line, "%lld %lld %lld", &M, &N, &NZ) == 3) break;
   if (M <= 0 || N != M) { fclose(f); return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("Matrix Market size line missing or matrix not square in ") + filename); }
   Comm           &cm = Comm::world();
   const long long lo = M * cm.rank / cm.size, hi = M * (cm.rank + 1) / cm.size;
   HYPRE_IJMatrixCreate(comm, lo, hi - 1, lo, hi - 1, matrix);
   HYPRE_IJMatrixInitialize(*matrix);
   auto *m   = *matrix;
   auto  put = [&](long long i, long long j, double v) {
      if (i < lo || i >= hi) return;
      m->t_row.push_back((int)(i - lo));
      m->t_col.push_back(j);
      m->t_val.push_back(v);
      m->t_add.push_back(1); // duplicate entries of a Matrix Market file are summed
   };
   long long got = 0;
   while (got < NZ && fgets(line, sizeof(line), f))
   {
      if (line[0] == '%' || line[0] == '\n') continue;
      long long i, j;
      double    v = 1.0;
      const int k = pattern ? sscanf(line, "%lld %lld", &i, &j) : sscanf(line, "%lld %lld %lf", &i, &j, &v);
      if (k != (pattern ? 2 : 3) || i < 1 || j < 1 || i > M || j > N || !std::isfinite(v))
      {
         fclose(f);
         return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("bad entry in Matrix Market file ") + filename);
      }
      got++;
      put(i - 1, j - 1, v);
      if ((sym || skew) && i != j) put(j - 1, i - 1, skew ? -v : v);
   }
   fclose(f);
   if (got != NZ) return hypre_set_error(HYPRE_ERROR_GENERIC, std::string("Matrix Market file ends early: ") + filename);
   return HYPRE_IJMatrixAssemble(m);
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_IJMatrixPrint(HYPRE_IJMatrix m, const char *filename)
{
   HY_TRY
   const std::string fn = rank_file(filename, Comm::world().rank);
   FILE             *f  = fopen(fn.c_str(), "w");
   if (!f) return hypre_set_error(HYPRE_ERROR_ARG, "cannot write " + fn);
   std::vector<int>    rp = m->A.rowptr.to_host(), cj((size_t)std::max(m->A.nnz, 1));
   std::vector<double> v((size_t)std::max(m->A.nnz, 1));
   if (m->A.nnz) { m->A.col.download(cj.data(), (size_t)m->A.nnz); m->A.val.download(v.data(), (size_t)m->A.nnz); }
   fprintf(f, "%lld %lld %lld %lld\n", m->ilower, m->iupper, m->jlower, m->jupper);
   const int ncl = (int)(m->jupper - m->jlower + 1);
   for (int i = 0; i < m->nloc; i++)
      for (int k = rp[(size_t)i]; k < rp[(size_t)i + 1]; k++)
      {
         const long long g = cj[(size_t)k] < ncl ? m->jlower + cj[(size_t)k] : m->ghost_gids[(size_t)(cj[(size_t)k] - ncl)];
         fprintf(f, "%lld %lld %.14e\n", m->ilower + i, g, v[(size_t)k]);
      }
   fclose(f);
   HY_CATCH
}

// ------------------------------------------------------------- ParCSR kernels

extern "C" HYPRE_Int HYPRE_ParCSRMatrixMatvec(HYPRE_Complex alpha, HYPRE_ParCSRMatrix A, HYPRE_ParVector x, HYPRE_Complex beta,
                                              HYPRE_ParVector y)
{
   HY_NEED_DEVICE;
   HY_TRY
   HDA_REQUIRE(A && A->assembled && x && y, "Matvec needs assembled operands");
   const double  *xin = x->cdata();
   DArray<double> xe;
   if (A->A.ncols > A->nloc || x->capacity < (size_t)A->A.ncols)
   { // stage x into an extended vector and refresh the ghost tail
      xe.alloc((size_t)std::max(A->A.ncols, 1));
      copy(A->nloc, x->cdata(), xe.data());
      halo_exchange(A->halo, xe.data());
      xin = xe.data();
   }
   double *yd = y->data();
   spmv(A->A, alpha, xin, beta, yd, yd);
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParVectorInnerProd(HYPRE_ParVector x, HYPRE_ParVector y, HYPRE_Real *prod)
{
   HY_NEED_DEVICE;
   HY_TRY
   if (x == y) { *prod = vector_self_dot(x); return 0; } // (one reduction per vector state: hda_hypre.h)
   dot(x->nloc, x->cdata(), y->cdata(), 0);
   finalize(0, S_TMP);
   *prod = read_scalar(S_TMP);
   HY_CATCH
}
// HYPRE_IJVectorInnerProd (hypre >= 2.32; examples/src/C_lidcavity/lidcavity.c:1404): the IJ handle is the ParVector here
extern "C" HYPRE_Int HYPRE_IJVectorInnerProd(HYPRE_IJVector x, HYPRE_IJVector y, HYPRE_Real *prod)
{
   if (!x || !y || !prod) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_IJVectorInnerProd: null argument");
   x->ensure_device();
   y->ensure_device();
   return HYPRE_ParVectorInnerProd(x, y, prod);
}
extern "C" HYPRE_Int HYPRE_ParVectorCopy(HYPRE_ParVector x, HYPRE_ParVector y)
{
   HY_TRY
   y->ensure_device();
   copy(x->nloc, x->cdata(), y->data());
   if (x->known_zero() && x->nloc == y->nloc && y->stage.empty()) y->mark_zero();
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParVectorScale(HYPRE_Complex a, HYPRE_ParVector x)
{
   HY_TRY
   scale(x->nloc, a, x->data());
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParVectorAxpy(HYPRE_Complex a, HYPRE_ParVector x, HYPRE_ParVector y)
{
   HY_TRY
   axpy(x->nloc, a, x->cdata(), y->data());
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParVectorSetConstantValues(HYPRE_ParVector v, HYPRE_Complex value)
{
   HY_NEED_DEVICE;
   HY_TRY
   v->ensure_device();
   std::vector<double>().swap(v->stage);
   fill(v->nloc, value, v->data());
   if (value == 0.0 && !std::signbit(value)) v->mark_zero();
   v->assembled = true;
   HY_CATCH
}

// --------------------------------------------------------------------- Krylov

static HYPRE_Int krylov_create(int kind, HYPRE_Solver *solver)
{
   auto *s = new hypre_Solver_struct();
   s->kind = kind;
   if (kind == HDA_SOLVER_GMRES || kind == HDA_SOLVER_FGMRES) s->kp.max_iter = 300; // src/internal/gmres.c:18, fgmres.c:17
   *solver = s;
   return 0;
}
extern "C" HYPRE_Int HYPRE_ParCSRPCGCreate(MPI_Comm, HYPRE_Solver *s) { return krylov_create(HDA_SOLVER_PCG, s); }
extern "C" HYPRE_Int HYPRE_ParCSRGMRESCreate(MPI_Comm, HYPRE_Solver *s) { return krylov_create(HDA_SOLVER_GMRES, s); }
extern "C" HYPRE_Int HYPRE_ParCSRFlexGMRESCreate(MPI_Comm, HYPRE_Solver *s) { return krylov_create(HDA_SOLVER_FGMRES, s); }
extern "C" HYPRE_Int HYPRE_ParCSRBiCGSTABCreate(MPI_Comm, HYPRE_Solver *s) { return krylov_create(HDA_SOLVER_BICGSTAB, s); }
extern "C" HYPRE_Int HYPRE_ParCSRFlexGMRESDestroy(HYPRE_Solver s) { delete s; return 0; }
extern "C" HYPRE_Int HYPRE_ParCSRBiCGSTABDestroy(HYPRE_Solver s) { delete s; return 0; }
extern "C" HYPRE_Int HYPRE_ParCSRPCGDestroy(HYPRE_Solver s) { delete s; return 0; }
extern "C" HYPRE_Int HYPRE_ParCSRGMRESDestroy(HYPRE_Solver s) { delete s; return 0; }

#define HY_SETTER(fn, type, stmt) \
   extern "C" HYPRE_Int fn(HYPRE_Solver s, type v) { if (!s) return hypre_set_error(HYPRE_ERROR_ARG, #fn ": null solver"); stmt; return 0; }

HY_SETTER(HYPRE_PCGSetMaxIter, HYPRE_Int, s->kp.max_iter = v)
HY_SETTER(HYPRE_PCGSetTwoNorm, HYPRE_Int, s->kp.two_norm = v)
HY_SETTER(HYPRE_PCGSetStopCrit, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_PCGSetRelChange, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_PCGSetPrintLevel, HYPRE_Int, s->kp.print_level = v)
HY_SETTER(HYPRE_PCGSetLogging, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_PCGSetRecomputeResidual, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_PCGSetTol, HYPRE_Real, s->kp.rtol = v)
HY_SETTER(HYPRE_PCGSetAbsoluteTol, HYPRE_Real, s->kp.atol = v)
HY_SETTER(HYPRE_PCGSetResidualTol, HYPRE_Real, (void)v)
HY_SETTER(HYPRE_PCGSetConvergenceFactorTol, HYPRE_Real, (void)v)
HY_SETTER(HYPRE_GMRESSetMinIter, HYPRE_Int, s->kp.min_iter = v)
HY_SETTER(HYPRE_GMRESSetMaxIter, HYPRE_Int, s->kp.max_iter = v)
HY_SETTER(HYPRE_GMRESSetStopCrit, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_GMRESSetSkipRealResidualCheck, HYPRE_Int, s->kp.skip_real_res_check = v)
HY_SETTER(HYPRE_GMRESSetKDim, HYPRE_Int, s->kp.krylov_dim = v)
HY_SETTER(HYPRE_GMRESSetRelChange, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_GMRESSetLogging, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_GMRESSetPrintLevel, HYPRE_Int, s->kp.print_level = v)
HY_SETTER(HYPRE_GMRESSetTol, HYPRE_Real, s->kp.rtol = v)
HY_SETTER(HYPRE_GMRESSetAbsoluteTol, HYPRE_Real, s->kp.atol = v)
HY_SETTER(HYPRE_GMRESSetConvergenceFactorTol, HYPRE_Real, (void)v)

// FlexGMRES (reference src/internal/fgmres.c:36-48) and BiCGSTAB (src/internal/bicgstab.c:41-55) setter sequences
HY_SETTER(HYPRE_FlexGMRESSetMinIter, HYPRE_Int, s->kp.min_iter = v)
HY_SETTER(HYPRE_FlexGMRESSetMaxIter, HYPRE_Int, s->kp.max_iter = v)
HY_SETTER(HYPRE_FlexGMRESSetKDim, HYPRE_Int, s->kp.krylov_dim = v)
HY_SETTER(HYPRE_FlexGMRESSetLogging, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_FlexGMRESSetPrintLevel, HYPRE_Int, s->kp.print_level = v)
HY_SETTER(HYPRE_FlexGMRESSetTol, HYPRE_Real, s->kp.rtol = v)
HY_SETTER(HYPRE_FlexGMRESSetAbsoluteTol, HYPRE_Real, s->kp.atol = v)
HY_SETTER(HYPRE_FlexGMRESSetConvergenceFactorTol, HYPRE_Real, (void)v)
HY_SETTER(HYPRE_BiCGSTABSetMinIter, HYPRE_Int, s->kp.min_iter = v)
HY_SETTER(HYPRE_BiCGSTABSetMaxIter, HYPRE_Int, s->kp.max_iter = v)
HY_SETTER(HYPRE_BiCGSTABSetStopCrit, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BiCGSTABSetLogging, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BiCGSTABSetPrintLevel, HYPRE_Int, s->kp.print_level = v)
HY_SETTER(HYPRE_BiCGSTABSetTol, HYPRE_Real, s->kp.rtol = v)
HY_SETTER(HYPRE_BiCGSTABSetAbsoluteTol, HYPRE_Real, s->kp.atol = v)
HY_SETTER(HYPRE_BiCGSTABSetConvergenceFactorTol, HYPRE_Real, (void)v)

static HYPRE_Int set_precond(HYPRE_Solver s, HYPRE_PtrToSolverFcn p, HYPRE_PtrToSolverFcn ps, HYPRE_Solver psolver)
{
   s->precond        = p;
   s->precond_setup  = ps;
   s->precond_solver = psolver;
   return 0;
}
extern "C" HYPRE_Int HYPRE_PCGSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn p, HYPRE_PtrToSolverFcn ps, HYPRE_Solver psolver)
{
   return set_precond(s, p, ps, psolver);
}
extern "C" HYPRE_Int HYPRE_GMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn p, HYPRE_PtrToSolverFcn ps, HYPRE_Solver psolver)
{
   return set_precond(s, p, ps, psolver);
}
extern "C" HYPRE_Int HYPRE_FlexGMRESSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn p, HYPRE_PtrToSolverFcn ps, HYPRE_Solver psolver)
{
   return set_precond(s, p, ps, psolver);
}
extern "C" HYPRE_Int HYPRE_BiCGSTABSetPrecond(HYPRE_Solver s, HYPRE_PtrToSolverFcn p, HYPRE_PtrToSolverFcn ps, HYPRE_Solver psolver)
{
   return set_precond(s, p, ps, psolver);
}

// hypre_PCGSetup / hypre_GMRESSetup: the only work is the preconditioner's setup callback
static HYPRE_Int krylov_setup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   HY_NEED_DEVICE;
   if (s->precond_setup) return s->precond_setup(s->precond_solver, A, b, x);
   return 0;
}
extern "C" HYPRE_Int HYPRE_ParCSRPCGSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_setup(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRGMRESSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_setup(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRFlexGMRESSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_setup(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRBiCGSTABSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_setup(s, A, b, x); }

namespace hda {
static std::unordered_set<const void *> &live_solvers()
{
   std::unordered_set<const void *> &s = RankState<std::unordered_set<const void *>>::get();
   return s;
}
void solver_registry(const void *p, int op)
{
   if (op > 0) live_solvers().insert(p);
   else live_solvers().erase(p);
}
bool is_live_solver(const void *p) { return p && live_solvers().count(p) != 0; }
} // namespace hda

#define g_precond_veclen (RankState<size_t, 3>::get())
extern "C" void hda_register_precond_veclen(size_t n) { g_precond_veclen = n; }
extern "C" void hda_reset_precond_veclen(void) { g_precond_veclen = 0; }

static HYPRE_Int krylov_solve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   HY_NEED_DEVICE;
   HY_TRY
   set_stage("Krylov solve");
   HDA_REQUIRE(A && A->assembled, "Krylov solve needs an assembled matrix");
   x->ensure_device();
   size_t veclen = g_precond_veclen;
   if (is_live_solver(s->precond_solver) && s->precond_solver->kind == HDA_SOLVER_AMG && s->precond_solver->pc.amg)
      veclen = std::max(veclen, s->precond_solver->pc.amg->vec_len0());
   LinOp     op(A->A, Comm::world().size > 1 ? &A->halo : nullptr, veclen);
   PrecondFn M;
   if (s->precond)
   {
      HYPRE_Solver         ps = s->precond_solver;
      HYPRE_PtrToSolverFcn fn = s->precond;
      const int            n  = A->nloc;
      const size_t         vl = op.veclen;
      M = [=](const double *r, double *z, int slot) {
         hypre_IJVector_struct vb, vx; // non-owning views for the C callback seam
         vb.nloc = vx.nloc = n;
         vb.jlower = vx.jlower = A->ilower;
         vb.jupper = vx.jupper = A->iupper;
         vb.view = const_cast<double *>(r);
         vx.view = z;
         vb.capacity = vx.capacity = vl;
         vb.assembled = vx.assembled = true;
         PrecondHints &h = precond_hints();
         h.zero_guess = true;
         h.dot_slot   = slot;
         h.dot_done   = false;
         const int ierr = fn(ps, A, &vb, &vx);
         const bool done = h.dot_done;
         h = PrecondHints();
         if (ierr) throw Error("preconditioner callback failed: " + hypre_last_error());
         if (slot >= 0 && !done) dot(n, r, z, slot);
      };
   }
   // what the vectors' counters know (hda_hypre.h), taken before x is handed over for writing: PCG starts from r = b when x is the
   // library's untouched zero fill, and shares <b,b> with the driver's r0 and relative residual
   PcgKnown known;
   if (s->kind == HDA_SOLVER_PCG && known_zero_enabled())
   {
      known.x_zero = x->known_zero() && x != b;
      if (s->kp.two_norm) known.bb = vector_self_dot(b);
   }
   const double *bd = b->cdata();
   double       *xd = x->data();
   s->last = (s->kind == HDA_SOLVER_GMRES)      ? gmres(op, M, s->kp, bd, xd)
             : (s->kind == HDA_SOLVER_FGMRES)   ? fgmres(op, M, s->kp, bd, xd)
             : (s->kind == HDA_SOLVER_BICGSTAB) ? bicgstab(op, M, s->kp, bd, xd)
                                                : pcg(op, M, s->kp, bd, xd, &known);
   if (!s->last.converged) g_hcode |= HYPRE_ERROR_CONV; // soft error, as in hypre
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParCSRPCGSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_solve(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRGMRESSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_solve(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRFlexGMRESSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_solve(s, A, b, x); }
extern "C" HYPRE_Int HYPRE_ParCSRBiCGSTABSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x) { return krylov_solve(s, A, b, x); }

#define HY_GETTER(fn, type, expr) \
   extern "C" HYPRE_Int fn(HYPRE_Solver s, type *out) { if (!s || !out) return hypre_set_error(HYPRE_ERROR_ARG, #fn ": null argument"); *out = (expr); return 0; }
HY_GETTER(HYPRE_PCGGetNumIterations, HYPRE_Int, s->last.iters)
HY_GETTER(HYPRE_PCGGetFinalRelativeResidualNorm, HYPRE_Real, s->last.final_rel)
HY_GETTER(HYPRE_PCGGetConverged, HYPRE_Int, s->last.converged ? 1 : 0)
HY_GETTER(HYPRE_GMRESGetNumIterations, HYPRE_Int, s->last.iters)
HY_GETTER(HYPRE_GMRESGetFinalRelativeResidualNorm, HYPRE_Real, s->last.final_rel)
HY_GETTER(HYPRE_GMRESGetConverged, HYPRE_Int, s->last.converged ? 1 : 0)
HY_GETTER(HYPRE_FlexGMRESGetNumIterations, HYPRE_Int, s->last.iters)
HY_GETTER(HYPRE_FlexGMRESGetFinalRelativeResidualNorm, HYPRE_Real, s->last.final_rel)
HY_GETTER(HYPRE_FlexGMRESGetConverged, HYPRE_Int, s->last.converged ? 1 : 0)
HY_GETTER(HYPRE_BiCGSTABGetNumIterations, HYPRE_Int, s->last.iters)
HY_GETTER(HYPRE_BiCGSTABGetFinalRelativeResidualNorm, HYPRE_Real, s->last.final_rel)
HY_GETTER(hypre_BiCGSTABGetConverged, HYPRE_Int, s->last.converged ? 1 : 0) // internal API the reference uses (solver.c:198-202)

// ------------------------------------------------------------------ BoomerAMG

extern "C" HYPRE_Int HYPRE_BoomerAMGCreate(HYPRE_Solver *solver)
{
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_AMG;
   // hypre's own defaults (not hypredrive's): 20 cycles, tol 1e-7, hybrid GS; hypredrive
   // overrides every one of them through the setter sequence of src/internal/amg.c:868-1032
   s->ap.max_iter = 20;
   s->ap.tol      = 1.0e-7;
   *solver        = s;
   return 0;
}
extern "C" HYPRE_Int HYPRE_BoomerAMGDestroy(HYPRE_Solver s)
{
   if (s)
   {
      try { if (have_device()) Context::get().sync(); } catch (...) {}
      delete s;
   }
   return 0;
}

HY_SETTER(HYPRE_BoomerAMGSetInterpType, HYPRE_Int, s->ap.interp_type = v)
HY_SETTER(HYPRE_BoomerAMGSetRestriction, HYPRE_Int, s->restriction = v)
HY_SETTER(HYPRE_BoomerAMGSetStrongThresholdR, HYPRE_Real, s->ap.restrict_strong_th = v)
HY_SETTER(HYPRE_BoomerAMGSetFilterThresholdR, HYPRE_Real, s->ap.restrict_filter_th = v)
HY_SETTER(HYPRE_BoomerAMGSetCoarsenType, HYPRE_Int, s->ap.coarsen_type = v)
HY_SETTER(HYPRE_BoomerAMGSetSabs, HYPRE_Int, s->sabs = v)
HY_SETTER(HYPRE_BoomerAMGSetTol, HYPRE_Real, s->ap.tol = v)
HY_SETTER(HYPRE_BoomerAMGSetStrongThreshold, HYPRE_Real, s->ap.strong_th = v)
HY_SETTER(HYPRE_BoomerAMGSetSeqThreshold, HYPRE_Int, s->seq_threshold = v)
HY_SETTER(HYPRE_BoomerAMGSetMaxCoarseSize, HYPRE_Int, s->ap.max_coarse_size = v)
HY_SETTER(HYPRE_BoomerAMGSetMinCoarseSize, HYPRE_Int, s->ap.min_coarse_size = v)
HY_SETTER(HYPRE_BoomerAMGSetTruncFactor, HYPRE_Real, s->ap.trunc_factor = v)
HY_SETTER(HYPRE_BoomerAMGSetPMaxElmts, HYPRE_Int, s->ap.pmax = v)
HY_SETTER(HYPRE_BoomerAMGSetPrintLevel, HYPRE_Int, s->ap.print_level = v)
HY_SETTER(HYPRE_BoomerAMGSetLogging, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BoomerAMGSetRelaxOrder, HYPRE_Int, s->relax_order = v)
HY_SETTER(HYPRE_BoomerAMGSetRelaxWt, HYPRE_Real, s->ap.relax_weight = v)
HY_SETTER(HYPRE_BoomerAMGSetOuterWt, HYPRE_Real, s->ap.outer_weight = v)
HY_SETTER(HYPRE_BoomerAMGSetCycleType, HYPRE_Int, s->cycle_type = v)
HY_SETTER(HYPRE_BoomerAMGSetMaxLevels, HYPRE_Int, s->ap.max_levels = v)
HY_SETTER(HYPRE_BoomerAMGSetMaxIter, HYPRE_Int, s->ap.max_iter = v)
HY_SETTER(HYPRE_BoomerAMGSetMaxRowSum, HYPRE_Real, s->ap.max_row_sum = v)
HY_SETTER(HYPRE_BoomerAMGSetNumFunctions, HYPRE_Int, s->num_functions = v)
// dof_func[i] in [0, num_functions) for the rows this rank owns; the array is COPIED (hypre takes
// ownership of a hypre_TAlloc'ed array instead -- reference src/internal/amg.c:792-862)
extern "C" HYPRE_Int HYPRE_BoomerAMGSetDofFunc(HYPRE_Solver s, HYPRE_Int *dof_func)
{
   HY_TRY
   HDA_REQUIRE(s && s->kind == HDA_SOLVER_AMG, "BoomerAMGSetDofFunc: not a BoomerAMG handle");
   s->dof_func_ptr = dof_func; // length is known at setup (local rows): copied there
   HY_CATCH
}
HY_SETTER(HYPRE_BoomerAMGSetFilterFunctions, HYPRE_Int, s->filter_functions = v)
HY_SETTER(HYPRE_BoomerAMGSetSmoothType, HYPRE_Int, s->smooth_type = v)
HY_SETTER(HYPRE_BoomerAMGSetSmoothNumSweeps, HYPRE_Int, s->ap.smooth_num_sweeps = v)
// ILU arguments of the complex smoother (reference src/internal/amg.c:903-921)
HY_SETTER(HYPRE_BoomerAMGSetILUType, HYPRE_Int, s->ilu_type = v)
HY_SETTER(HYPRE_BoomerAMGSetILULevel, HYPRE_Int, s->ilu_fill = v)
HY_SETTER(HYPRE_BoomerAMGSetILULocalReordering, HYPRE_Int, s->ilu_reordering = v)
HY_SETTER(HYPRE_BoomerAMGSetILUTriSolve, HYPRE_Int, s->ilup.tri_solve = v)
HY_SETTER(HYPRE_BoomerAMGSetILULowerJacobiIters, HYPRE_Int, s->ilup.lower_it = v)
HY_SETTER(HYPRE_BoomerAMGSetILUUpperJacobiIters, HYPRE_Int, s->ilup.upper_it = v)
HY_SETTER(HYPRE_BoomerAMGSetILUDroptol, HYPRE_Real, (void)v)   // threshold variants (ilut) only
HY_SETTER(HYPRE_BoomerAMGSetILUMaxRowNnz, HYPRE_Int, (void)v)  // threshold variants only
HY_SETTER(HYPRE_BoomerAMGSetILUMaxIter, HYPRE_Int, s->ap.smooth_num_sweeps = v) // amg.c:921 passes smoother.num_sweeps
HY_SETTER(HYPRE_BoomerAMGSetSmoothNumLevels, HYPRE_Int, s->smooth_num_levels = v)
// aggressive coarsening (reference src/internal/amg.c:938-944): levels, paths, the multipass interpolation (4) and the two-stage
// mm_extended (5) / mm_extended+i (6) interpolations with their P12 truncation are built (hda_amg_agg.hip); the other two-stage types
// (1, 2, 3, 7) are refused by name at Setup
HY_SETTER(HYPRE_BoomerAMGSetAggNumLevels, HYPRE_Int, s->agg_num_levels = v)
HY_SETTER(HYPRE_BoomerAMGSetAggInterpType, HYPRE_Int, s->ap.agg_interp_type = v)
HY_SETTER(HYPRE_BoomerAMGSetAggTruncFactor, HYPRE_Real, s->agg_trunc[0] = v)
HY_SETTER(HYPRE_BoomerAMGSetAggP12TruncFactor, HYPRE_Real, s->agg_trunc[1] = v)
HY_SETTER(HYPRE_BoomerAMGSetAggPMaxElmts, HYPRE_Int, s->agg_trunc[2] = v)
HY_SETTER(HYPRE_BoomerAMGSetAggP12MaxElmts, HYPRE_Int, s->agg_trunc[3] = v)
HY_SETTER(HYPRE_BoomerAMGSetNumPaths, HYPRE_Int, s->ap.agg_num_paths = v)
HY_SETTER(HYPRE_BoomerAMGSetRAP2, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BoomerAMGSetModuleRAP2, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BoomerAMGSetKeepTranspose, HYPRE_Int, (void)v)
HY_SETTER(HYPRE_BoomerAMGSetChebyOrder, HYPRE_Int, s->ap.cheby_order = v)
HY_SETTER(HYPRE_BoomerAMGSetChebyFraction, HYPRE_Real, s->ap.cheby_fraction = v)
HY_SETTER(HYPRE_BoomerAMGSetChebyEigEst, HYPRE_Int, s->ap.cheby_eig_est = v)
HY_SETTER(HYPRE_BoomerAMGSetChebyVariant, HYPRE_Int, s->ap.cheby_variant = v)
HY_SETTER(HYPRE_BoomerAMGSetChebyScale, HYPRE_Int, s->ap.cheby_scale = v)

extern "C" HYPRE_Int HYPRE_BoomerAMGSetRelaxType(HYPRE_Solver s, HYPRE_Int t)
{
   s->ap.relax_down = s->ap.relax_up = t;
   s->ap.relax_coarse = 9;
   s->relax_type_all  = t;
   return 0;
}
extern "C" HYPRE_Int HYPRE_BoomerAMGSetCycleRelaxType(HYPRE_Solver s, HYPRE_Int t, HYPRE_Int k)
{
   if (k == 1) s->ap.relax_down = t;
   else if (k == 2) s->ap.relax_up = t;
   else if (k == 3) s->ap.relax_coarse = t;
   else return hypre_set_error(HYPRE_ERROR_ARG, "SetCycleRelaxType: k must be 1, 2 or 3");
   return 0;
}
extern "C" HYPRE_Int HYPRE_BoomerAMGSetNumSweeps(HYPRE_Solver s, HYPRE_Int n)
{
   s->ap.sweeps_down = s->ap.sweeps_up = n;
   s->ap.sweeps_coarse = 1;
   return 0;
}
extern "C" HYPRE_Int HYPRE_BoomerAMGSetCycleNumSweeps(HYPRE_Solver s, HYPRE_Int n, HYPRE_Int k)
{
   if (k == 1) s->ap.sweeps_down = n;
   else if (k == 2) s->ap.sweeps_up = n;
   else if (k == 3) s->ap.sweeps_coarse = n;
   else return hypre_set_error(HYPRE_ERROR_ARG, "SetCycleNumSweeps: k must be 1, 2 or 3");
   return 0;
}

// the points every sweep relaxes (reference amg.c:988-1015 builds the AIR schedule): [1] down, [2] up, [3] coarsest, one entry per sweep
// of the counts set so far ([0] unused, as in hypre).  Copied: hypre takes the arrays over, this library does not.  NULL is refused
// as in hypre; the schedule itself is checked at Setup
extern "C" HYPRE_Int HYPRE_BoomerAMGSetGridRelaxPoints(HYPRE_Solver s, HYPRE_Int **pts)
{
   if (!s) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_BoomerAMGSetGridRelaxPoints: null solver");
   if (!pts) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_BoomerAMGSetGridRelaxPoints: null grid_relax_points");
   const int ns[3] = {std::max(s->ap.sweeps_down, 0), std::max(s->ap.sweeps_up, 0), std::max(s->ap.sweeps_coarse, 0)};
   for (int k = 0; k < 3; k++)
      if (ns[k] > 0 && !pts[k + 1]) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_BoomerAMGSetGridRelaxPoints: a direction with sweeps has no points");
   for (int k = 0; k < 3; k++) s->grid_points[k].assign(pts[k + 1], pts[k + 1] + ns[k]);
   s->grid_points_set = true;
   return 0;
}

extern "C" HYPRE_Int HYPRE_BoomerAMGSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_NEED_DEVICE;
   HY_TRY
   set_stage("preconditioner setup (HYPRE_BoomerAMGSetup)");
   HDA_REQUIRE(s && s->kind == HDA_SOLVER_AMG, "BoomerAMGSetup: not a BoomerAMG handle");
   HDA_REQUIRE(A && A->assembled, "BoomerAMGSetup needs an assembled matrix");
   // features of the reference's parameter surface that this build does not implement
   s->ap.agg_num_levels = std::max(s->agg_num_levels, 0);
   if (s->ap.agg_num_levels > 0)
   {
      HDA_REQUIRE(amg_agg_interp_type_built(s->ap.agg_interp_type), amg_agg_interp_refusal(s->ap.agg_interp_type).c_str());
      s->ap.agg_trunc_factor = s->agg_trunc[0];
      s->ap.agg_pmax         = (int)s->agg_trunc[2];
      // P12_*: the first stage of the two-stage types (5 / 6); accepted and unused with multipass, as in hypre
      s->ap.agg_p12_trunc_factor = s->agg_trunc[1];
      s->ap.agg_p12_pmax         = (int)s->agg_trunc[3];
   }
   if (s->smooth_num_levels > 0)
   {
      const std::string built = "complex smoother: ILU (smoother.type: ilu) and static FSAI (smoother.type: fsai with fsai.algo_type: bj-sfsai) are "
                                "implemented on MI355X; ";
      if (s->smooth_type != 5 && s->smooth_type != 4) throw Error(built + "Schwarz, Pilut, ParaSails and Euclid are not");
      if (s->smooth_type == 4)
      { // (max_iter, tolerance and print_level of the smoother's fsai block are not forwarded by amg.c:924-932: one step is num_sweeps iterations)
         FsaiParams fp = s->fsaip;
         fp.max_iter   = 1;
         const std::string why = fsai_refusal(s->fs_algo, fp, 0.0);
         if (!why.empty()) throw Error(built + why);
         HDA_REQUIRE(Comm::world().size == 1, "complex smoother: FSAI in a world of more than one rank is not implemented (the pattern of a row partition "
                                              "needs off-rank rows of the power of A); one rank with HDA_BLOCKS row blocks is");
      }
      else
         HDA_REQUIRE(s->ilu_type == 0 && s->ilu_fill == 0 && s->ilu_reordering == 0,
                     "ILU smoother: only type bj-iluk with fill_level 0 and reordering 0 is implemented");
   }
   s->ap.fsai.num_levels = s->fsaip.num_levels; s->ap.fsai.max_nnz_row = s->fsaip.max_nnz_row; s->ap.fsai.eig_max_iters = s->fsaip.eig_max_iters;
   s->ap.fsai.threshold  = s->fsaip.threshold;
   s->ap.smooth_type       = s->smooth_type;
   s->ap.smooth_num_levels = std::max(s->smooth_num_levels, 0);
   s->ap.ilu               = s->ilup;
   HDA_REQUIRE(s->cycle_type == 1, "only V-cycles (cycle type 1) are implemented");
   HDA_REQUIRE(s->filter_functions == 0 || s->num_functions <= 1, "coarsening.filter_functions is not implemented for systems AMG");
   HDA_REQUIRE(s->restriction != 3 && s->restriction != 4 && s->restriction != 5 && s->restriction != 15,
               "restriction_type: neumann_air_0/1/2 (3, 4, 5) and air_1.5 (15) are not implemented; p_transpose (0), air_1 (1) and air_2 (2) are");
   HDA_REQUIRE(s->restriction >= 0 && s->restriction <= 2, "restriction_type: p_transpose (0), air_1 (1) and air_2 (2) are implemented");
   s->ap.restrict_type = s->restriction;
   s->ap.points_down.clear();
   s->ap.points_up.clear();
   if (s->grid_points_set)
   { // the schedule: all points on the coarsest level, all / F / C points on every down and up sweep
      HDA_REQUIRE((int)s->grid_points[0].size() == std::max(s->ap.sweeps_down, 0) && (int)s->grid_points[1].size() == std::max(s->ap.sweeps_up, 0) &&
                      (int)s->grid_points[2].size() == std::max(s->ap.sweeps_coarse, 0),
                  "relaxation points (HYPRE_BoomerAMGSetGridRelaxPoints) were set for other sweep counts than the cycle has");
      for (int p : s->grid_points[2])
         HDA_REQUIRE(p == 0, "relaxation points: the coarsest level relaxes all points (F- or C-point sweeps there are not implemented)");
      for (int k = 0; k < 2; k++)
         for (int p : s->grid_points[k])
            HDA_REQUIRE(p >= -1 && p <= 1, "relaxation points: every down / up sweep relaxes all (0), F (-1) or C (1) points");
      s->ap.points_down = s->grid_points[0];
      s->ap.points_up   = s->grid_points[1];
   }
   HDA_REQUIRE(s->relax_order == 0, "only lexicographic relaxation order (relaxation.order 0) is implemented");
   s->ap.num_functions = std::max(s->num_functions, 1);
   // row blocks (the reference's hybrid Gauss-Seidel / HMIS at np = V on one GPU): HDA_BLOCKS = V, 1 = the sequential algorithms,
   // unset = the setup's own choice (one block up to HDA_BLOCKS_MIN_ROWS rows); across ranks the rank blocks are the blocks
   s->ap.blocks = (Comm::world().size > 1) ? 1 : env_blocks(0);
   s->pc.owned_amg = std::make_unique<Amg>(s->ap);
   s->pc.amg       = s->pc.owned_amg.get();
   s->pc.kind      = Precond::AMG;
   if (s->ap.num_functions > 1)
   {
      if (s->dof_func_ptr) s->pc.amg->dof_func0.assign(s->dof_func_ptr, s->dof_func_ptr + A->nloc);
      s->pc.amg->dof_row_offset = A->ilower; // hypre's default: (global row) mod num_functions
   }
   if (Comm::world().size > 1)
   {
      // partitioned (default): every setup phase works on the row blocks; replicated
      // (HDA_DIST_SETUP=replicated): every rank builds the whole hierarchy and keeps its rows --
      // the specification the partitioned setup is checked against (HDA_DIST_CHECK=1)
      const char *mode = getenv("HDA_DIST_SETUP");
      // (HMIS = sequential Ruge pass: only the replicated scheme can run it, on the gathered operator)
      // (approximate ideal restriction: a neighbourhood reaches past the rank's rows -- hypre fetches the off-rank rows -- and F / C
      //  sweeps need every level's splitting: both are built on the gathered operator)
      // (aggressive levels: their second strength graph reaches two ghost layers deep -- built on the gathered operator too)
      // (mm-ext+i, type 17: its sparse products are formed on the gathered operator as well; direct (3) and standard (8) interpolation:
      //  options beside the path, one-rank kernels; so are extended (14), mm-ext (16), one-point (100) and multipass (4))
      if ((mode && !strcmp(mode, "replicated")) || s->ap.coarsen_type != 8 || s->ap.num_functions > 1 || s->ap.smooth_num_levels > 1 || s->ap.agg_num_levels > 0 ||
          s->ap.interp_type != 6 || s->ap.restrict_type != 0 || !s->ap.points_down.empty() || !s->ap.points_up.empty())
         s->pc.amg->setup_dist(A->A, A->halo, A->part, A->ghost_gids);
      else s->pc.amg->setup_dist_partitioned(A->A, A->halo, A->part, A->ghost_gids);
   }
   else s->pc.amg->setup(A->A);
   hda_register_precond_veclen(s->pc.amg->vec_len0());
   if (s->ap.print_level > 0 && Comm::world().rank == 0)
   {
      printf("\n BoomerAMG (MI355X): %d levels, grid complexity %.6f, operator complexity %.6f\n", s->pc.amg->num_levels(),
             s->pc.amg->grid_complexity(), s->pc.amg->operator_complexity());
      printf(" coarsening %s (%d)\n", amg_coarsen_name(s->ap.coarsen_type) ? amg_coarsen_name(s->ap.coarsen_type) : "?", s->ap.coarsen_type);
      if (s->pc.amg->blocks_used > 1)
         printf(" %d row blocks (hybrid Gauss-Seidel / HMIS / RS / Falgout as on %d ranks)\n", s->pc.amg->blocks_used, s->pc.amg->blocks_used);
      printf("\n");
   }
   HY_CATCH
}

// body(xp) on the iterate of x with room for `need` entries: x's own buffer when it is that long, otherwise a temporary with the owned
// part copied in before and out after (a caller's vector holds its owned entries; level-0 vectors of a row block carry ghosts behind them)
template <class Body>
static void with_room(HYPRE_ParVector x, int nloc, size_t need, Body body)
{
   if (x->capacity >= need) { body(x->data()); return; }
   DArray<double> xe(need);
   copy(nloc, x->data(), xe.data());
   body(xe.data());
   copy(nloc, xe.data(), x->data());
}
// HYPRE_{ILU,Schwarz,FSAI,AMS,MGR}Solve: the kind's own checks of the handle (and MGR's rebind), then its solve from the guess the Krylov
// loop's hint names.  stage: the iterate gets room for the kind's level-0 vectors (the kinds that run on row partitions)
template <class Check>
static HYPRE_Int precond_solve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x, bool stage, Check check)
{
   HY_NEED_DEVICE;
   HY_TRY
   check();
   x->ensure_device();
   const bool      zero = precond_hints().zero_guess;
   const HaloPlan *halo = Comm::world().size > 1 ? &A->halo : nullptr;
   auto            body = [&](double *xp) { s->pc.solve(A->A, halo, b->data(), xp, zero); };
   if (stage) with_room(x, A->nloc, s->pc.vec_len(A->A), body);
   else body(x->data());
   s->amg_iters = s->pc.iterations();
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_BoomerAMGSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   HY_NEED_DEVICE;
   HY_TRY
   HDA_REQUIRE(s && s->pc.amg, "BoomerAMGSolve before BoomerAMGSetup");
   if (!s->pc.amg->bound_to(A->A)) s->pc.amg->rebind(A->A, Comm::world().size > 1 ? &A->halo : nullptr); // reused hierarchy, later system
   x->ensure_device();
   PrecondHints &h    = precond_hints();
   const size_t  need = s->pc.amg->vec_len0();
   with_room(x, A->nloc, need, [&](double *xp) {
      if (h.zero_guess && s->ap.max_iter == 1)
      {
         s->pc.amg->apply_offering(b->data(), xp, h.dot_slot); // (honours and renews the first-sweep offer of PCG)
         if (h.dot_slot >= 0) h.dot_done = true;
         s->amg_iters = 1;
      }
      else
      {
         // stand-alone solver use: up to max_iter cycles, optional relative residual test
         double bn = 0.0;
         DArray<double> r, xs;
         if (s->ap.tol > 0.0)
         {
            dot(A->nloc, b->data(), b->data(), 0);
            finalize(0, S_TMP);
            bn = std::sqrt(read_scalar(S_TMP));
            r.alloc((size_t)std::max(A->nloc, 1));
            xs.alloc(std::max(need, (size_t)A->A.ncols));
         }
         AmgParams one = s->pc.amg->prm;
         s->amg_iters  = 0;
         for (int it = 0; it < std::max(s->ap.max_iter, 1); it++)
         {
            s->pc.amg->prm.max_iter = 1;
            s->pc.amg->solve(b->data(), xp);
            s->amg_iters++;
            if (s->ap.tol > 0.0)
            {
               copy(A->nloc, xp, xs.data());
               halo_exchange(A->halo, xs.data());
               residual(A->A, xs.data(), b->data(), r.data());
               dot(A->nloc, r.data(), r.data(), 0);
               finalize(0, S_TMP);
               s->amg_rel = std::sqrt(read_scalar(S_TMP)) / (bn > 0.0 ? bn : 1.0);
               if (s->amg_rel <= s->ap.tol) break;
            }
         }
         s->pc.amg->prm = one;
         if (s->ap.tol > 0.0) gs_free_check(); // (stand-alone solver with a residual test: the host is in step anyway -- report an aborted block sweep here)
      }
   });
   HY_CATCH
}
// ------------------------------------------------------------------------ ILU
// HYPRE_ILU* as driven by hypredrv_ILUCreate (reference src/internal/ilu.c:63-115) and the
// precon_ops table (src/internal/precon.c).  Implemented: type 0 (bj-iluk), fill level 0, no reordering.

extern "C" HYPRE_Int HYPRE_ILUCreate(HYPRE_Solver *solver)
{
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_ILU;
   s->ilup.max_iter = 20; // hypre's own default; hypredrive sets 1 (ilu.c:17)
   *solver = s;
   return 0;
}
extern "C" HYPRE_Int HYPRE_ILUDestroy(HYPRE_Solver s) { return HYPRE_BoomerAMGDestroy(s); }
HY_SETTER(HYPRE_ILUSetType, HYPRE_Int, s->ilu_type = v)
HY_SETTER(HYPRE_ILUSetLevelOfFill, HYPRE_Int, s->ilu_fill = v)
HY_SETTER(HYPRE_ILUSetLocalReordering, HYPRE_Int, s->ilu_reordering = v)
HY_SETTER(HYPRE_ILUSetTriSolve, HYPRE_Int, s->ilup.tri_solve = v)
HY_SETTER(HYPRE_ILUSetLowerJacobiIters, HYPRE_Int, s->ilup.lower_it = v)
HY_SETTER(HYPRE_ILUSetUpperJacobiIters, HYPRE_Int, s->ilup.upper_it = v)
HY_SETTER(HYPRE_ILUSetPrintLevel, HYPRE_Int, s->ap.print_level = v)
HY_SETTER(HYPRE_ILUSetMaxIter, HYPRE_Int, s->ilup.max_iter = v)
HY_SETTER(HYPRE_ILUSetTol, HYPRE_Real, s->ap.tol = v)
HY_SETTER(HYPRE_ILUSetMaxNnzPerRow, HYPRE_Int, (void)v)     // threshold variants only
HY_SETTER(HYPRE_ILUSetDropThreshold, HYPRE_Real, (void)v)   // threshold variants only
HY_SETTER(HYPRE_ILUSetSchurMaxIter, HYPRE_Int, (void)v)     // Schur-complement variants only
HY_SETTER(HYPRE_ILUSetNSHDropThreshold, HYPRE_Real, (void)v)

extern "C" HYPRE_Int HYPRE_ILUSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_NEED_DEVICE;
   HY_TRY
   HDA_REQUIRE(s && s->kind == HDA_SOLVER_ILU, "ILUSetup: not an ILU handle");
   HDA_REQUIRE(A && A->assembled, "ILUSetup needs an assembled matrix");
   HDA_REQUIRE(s->ilu_type == 0, "ILU: only type bj-iluk (0) is implemented on MI355X; ilut / gmres- / nsh- / ras- / ddpq- variants are not");
   HDA_REQUIRE(s->ilu_fill == 0, "ILU: only fill_level 0 is implemented");
   HDA_REQUIRE(s->ilu_reordering == 0, "ILU: only reordering 0 (natural order) is implemented");
   s->pc.kind = Precond::ILU;
   s->pc.ilu  = std::make_unique<Ilu>();
   // `preconditioner: ilu` factors the WHOLE matrix of a rank, as the reference does at np = 1 (round-4 ADVICE: the automatic row
   // blocks made it block-Jacobi ILU silently, dropping every coupling between blocks).  Row blocks (bj-iluk at np = V on one GPU;
   // the exact substitutions then run as block sweeps) are opt-in: HDA_BLOCKS = V, 0 = the setup's own choice; always said.
   s->ilup.blocks = (Comm::world().size > 1 || !s->ilup.tri_solve) ? 1 : env_blocks(1);
   s->pc.ilu->setup(A->A, s->ilup);
   if (Comm::world().rank == 0 && s->pc.ilu->blocks_used() > 1 && !quiet())
      fprintf(stderr, "[hypredrv_amd] ILU(0): %d row blocks (HDA_BLOCKS): block-Jacobi ILU as the reference computes it on %d ranks; couplings between blocks are dropped\n",
              s->pc.ilu->blocks_used(), s->pc.ilu->blocks_used());
   hda_register_precond_veclen((size_t)std::max(A->A.ncols, A->A.nrows));
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_ILUSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return precond_solve(s, A, b, x, true, [&] { HDA_REQUIRE(s && s->pc.ilu, "ILUSolve before ILUSetup"); });
}
HY_GETTER(HYPRE_ILUGetNumIterations, HYPRE_Int, s->amg_iters)
HY_GETTER(HYPRE_ILUGetFinalRelativeResidualNorm, HYPRE_Real, s->amg_rel)

// ------------------------------------------------------------------------ Schwarz
// HYPRE_Schwarz* as driven by hypredrv_SchwarzCreate (reference src/internal/schwarz.c:82-96).  Built (hda_schwarz.hip): variants 10
// (ras-iluk) and 11 (as-iluk) with ILU(k) subdomain solves on one rank; everything else is refused by name at Setup.
namespace hda {
std::string schwarz_refusal(int variant, int local_solver, int overlap, int fill, int max_iter, double tol, int num_functions, int domain_type,
                            int nonsymm)
{
   static const std::pair<int, const char *> names[] = {{0, "mp"}, {1, "ad"}, {2, "par-ad"}, {3, "par-mp"}, {4, "mp-fw"}, {10, "ras-iluk"},
                                                        {11, "as-iluk"}, {20, "ras-ilut"}, {21, "as-ilut"}, {30, "ras-amg"}, {31, "as-amg"},
                                                        {40, "ras-spdirect"}, {41, "as-spdirect"}};
   static const char *solvers[] = {"iluk", "ilut", "amg", "spdirect"};
   if (variant != 10 && variant != 11)
   {
      std::string nm = std::to_string(variant);
      for (auto &q : names)
         if (q.first == variant) nm = std::string("'") + q.second + "' (" + std::to_string(variant) + ")";
      return "Schwarz: variant " + nm + " is not implemented on MI355X; ras-iluk (10) and as-iluk (11) are";
   }
   if (local_solver != 0)
      return std::string("Schwarz: local_solver_type '") + (local_solver >= 0 && local_solver < 4 ? solvers[local_solver] : "?") +
             "' contradicts variant " + (variant == 10 ? "ras-iluk" : "as-iluk") + ", whose subdomain solver is iluk";
   if (tol != 0.0) return "Schwarz: tolerance != 0 (a residual test inside the preconditioner) is not implemented; max_iter fixed iterations are";
   if (num_functions != 1) return "Schwarz: num_functions " + std::to_string(num_functions) + " is not implemented (1 only)";
   if (domain_type != 2) return "Schwarz: domain_type " + std::to_string(domain_type) + " is not implemented (2, the default: one subdomain per row block, only)";
   if (nonsymm != 0) return "Schwarz: use_nonsymm " + std::to_string(nonsymm) + " is not implemented (0 only)";
   if (overlap < 0) return "Schwarz: overlap must be >= 0";
   if (fill < 0) return "Schwarz: iluk_level_of_fill must be >= 0";
   if (max_iter < 1) return "Schwarz: max_iter must be >= 1";
   return std::string();
}
} // namespace hda

extern "C" HYPRE_Int HYPRE_SchwarzCreate(HYPRE_Solver *solver)
{
   if (!solver) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_SchwarzCreate: null output");
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_SCHWARZ;
   *solver = s;
   return 0;
}
// (precon.c:138-154 calls this for whatever handle its table holds: NULL is fine, a handle of another kind is not a Schwarz handle)
extern "C" HYPRE_Int HYPRE_SchwarzDestroy(HYPRE_Solver s)
{
   if (!s) return 0;
   if (!is_live_solver(s) || s->kind != HDA_SOLVER_SCHWARZ) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_SchwarzDestroy: not a Schwarz handle");
   return HYPRE_BoomerAMGDestroy(s);
}
HY_SETTER(HYPRE_SchwarzSetVariant, HYPRE_Int, s->sw_variant = v)
HY_SETTER(HYPRE_SchwarzSetOverlap, HYPRE_Int, s->sw_overlap = v)
HY_SETTER(HYPRE_SchwarzSetDomainType, HYPRE_Int, s->sw_domain_type = v)
HY_SETTER(HYPRE_SchwarzSetRelaxWeight, HYPRE_Real, s->sw_weight = v)
HY_SETTER(HYPRE_SchwarzSetNumFunctions, HYPRE_Int, s->sw_num_functions = v)
HY_SETTER(HYPRE_SchwarzSetNonSymm, HYPRE_Int, s->sw_nonsymm = v)
HY_SETTER(HYPRE_SchwarzSetLocalSolverType, HYPRE_Int, s->sw_local_solver = v)
HY_SETTER(HYPRE_SchwarzSetILUKLevelOfFill, HYPRE_Int, s->sw_fill = v)
HY_SETTER(HYPRE_SchwarzSetILUTMaxNnzPerRow, HYPRE_Int, (void)v) // threshold variants only (refused at Setup by their variant)
HY_SETTER(HYPRE_SchwarzSetILUTDroptol, HYPRE_Real, (void)v)    // threshold variants only
HY_SETTER(HYPRE_SchwarzSetMaxIter, HYPRE_Int, s->sw_max_iter = v)
HY_SETTER(HYPRE_SchwarzSetTol, HYPRE_Real, s->sw_tol = v)
HY_SETTER(HYPRE_SchwarzSetPrintLevel, HYPRE_Int, s->sw_print_level = v)
HY_SETTER(HYPRE_SchwarzSetLogging, HYPRE_Int, s->sw_logging = v) // (nothing is logged beyond the print_level line)

extern "C" HYPRE_Int HYPRE_SchwarzSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_TRY
   HDA_REQUIRE(s && is_live_solver(s) && s->kind == HDA_SOLVER_SCHWARZ, "SchwarzSetup: not a Schwarz handle");
   const std::string why = schwarz_refusal(s->sw_variant, s->sw_local_solver, s->sw_overlap, s->sw_fill, s->sw_max_iter, s->sw_tol,
                                           s->sw_num_functions, s->sw_domain_type, s->sw_nonsymm);
   if (!why.empty()) throw Error(why);
   HDA_REQUIRE(Comm::world().size == 1, "Schwarz: a world of more than one rank is not implemented (subdomains across row partitions need off-rank rows); "
                                        "one rank with HDA_BLOCKS row blocks is");
   if (!have_device()) throw Error("no HIP device visible: the MI355X solve path has no CPU fallback");
   HDA_REQUIRE(A && A->assembled, "SchwarzSetup needs an assembled matrix");
   SchwarzParams p;
   p.variant = s->sw_variant - 10; p.overlap = s->sw_overlap; p.fill = s->sw_fill; p.max_iter = s->sw_max_iter; p.weight = s->sw_weight;
   // one subdomain per rank is hypre's picture; on one GPU the row blocks play the ranks (HDA_BLOCKS = V, 0 = the setup's choice), as for ILU
   p.blocks  = env_blocks(1);
   s->pc.kind    = Precond::SCHWARZ;
   s->pc.schwarz = std::make_unique<Schwarz>();
   s->pc.schwarz->setup(A->A, p);
   const Schwarz &S = *s->pc.schwarz;
   if (S.V > 1 && !quiet())
      fprintf(stderr, "[hypredrv_amd] Schwarz: %d row blocks (HDA_BLOCKS): one subdomain per block, as the reference has one per rank on %d ranks\n", S.V, S.V);
   if (s->sw_print_level >= 1)
      printf("Schwarz (%s): %d subdomains, overlap %d, N_ext / n = %.3f, ILU(%d), nnz(LU) / nnz(A) = %.3f\n", s->sw_variant == 10 ? "ras-iluk" : "as-iluk",
             S.V, p.overlap, S.n ? (double)S.n_ext / S.n : 1.0, p.fill, S.nnz_A ? (double)S.factors().nnz / (double)S.nnz_A : 1.0);
   hda_register_precond_veclen((size_t)std::max(A->A.ncols, A->A.nrows));
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_SchwarzSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return precond_solve(s, A, b, x, false, [&] { HDA_REQUIRE(s && s->pc.schwarz, "SchwarzSolve before SchwarzSetup"); });
}

// ------------------------------------------------------------------------ FSAI
// HYPRE_FSAI* as driven by hypredrv_FSAICreate (reference src/internal/fsai.c:71-86).  Built (hda_fsai.hip): the static
// algorithm, algo_type 3 (bj-sfsai), on one rank with HDA_BLOCKS row blocks.  The adaptive algorithms 1 and 2 -- the reference's default --
// are host algorithms in hypre and are not built; a handle's algo_type starts at 1 as in the reference, so nothing runs another algorithm
// than the one named.
namespace hda {
std::string fsai_refusal(int algo_type, const FsaiParams &p, double tol)
{
   if (algo_type != 3)
   {
      const char *nm = algo_type == 1 ? "bj-afsai (1)" : algo_type == 2 ? "bj-afsai-omp (2)" : nullptr;
      return "FSAI: algo_type " + (nm ? std::string(nm) : std::to_string(algo_type)) +
             " is not implemented on MI355X (the adaptive algorithms, the reference's default, are host algorithms); algo_type bj-sfsai (3), the static "
             "pattern, is built";
   }
   if (tol != 0.0) return "FSAI: tolerance != 0 (a residual test inside the preconditioner) is not implemented; max_iter fixed iterations are";
   return fsai_params_refusal(p);
}
} // namespace hda

extern "C" HYPRE_Int HYPRE_FSAICreate(HYPRE_Solver *solver)
{
   if (!solver) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_FSAICreate: null output");
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_FSAI;
   *solver = s;
   return 0;
}
// (precon.c:138-154 calls this for whatever handle its table holds: NULL is fine, a handle of another kind is not an FSAI handle)
extern "C" HYPRE_Int HYPRE_FSAIDestroy(HYPRE_Solver s)
{
   if (!s) return 0;
   if (!is_live_solver(s) || s->kind != HDA_SOLVER_FSAI) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_FSAIDestroy: not an FSAI handle");
   return HYPRE_BoomerAMGDestroy(s);
}
HY_SETTER(HYPRE_FSAISetAlgoType, HYPRE_Int, s->fs_algo = v)
HY_SETTER(HYPRE_FSAISetLocalSolveType, HYPRE_Int, s->fs_ls_type = v)    // adaptive algorithms only: recorded, unused
HY_SETTER(HYPRE_FSAISetMaxSteps, HYPRE_Int, s->fs_max_steps = v)        // adaptive algorithms only
HY_SETTER(HYPRE_FSAISetMaxStepSize, HYPRE_Int, s->fs_max_step_size = v) // adaptive algorithms only
HY_SETTER(HYPRE_FSAISetMaxNnzRow, HYPRE_Int, s->fsaip.max_nnz_row = v)
HY_SETTER(HYPRE_FSAISetNumLevels, HYPRE_Int, s->fsaip.num_levels = v)
HY_SETTER(HYPRE_FSAISetEigMaxIters, HYPRE_Int, s->fsaip.eig_max_iters = v)
HY_SETTER(HYPRE_FSAISetThreshold, HYPRE_Real, s->fsaip.threshold = v)
HY_SETTER(HYPRE_FSAISetKapTolerance, HYPRE_Real, s->fs_kap_tol = v)     // adaptive algorithms only
HY_SETTER(HYPRE_FSAISetMaxIterations, HYPRE_Int, s->fsaip.max_iter = v)
HY_SETTER(HYPRE_FSAISetTolerance, HYPRE_Real, s->fs_tol = v)
HY_SETTER(HYPRE_FSAISetPrintLevel, HYPRE_Int, s->fs_print_level = v)
// the same nine numbers for BoomerAMG's FSAI smoother (amg.c:924-932 calls these for EVERY BoomerAMG whatever its smoother: they record
// and succeed; what they name is checked by HYPRE_BoomerAMGSetup when smooth_type is 4)
HY_SETTER(HYPRE_BoomerAMGSetFSAIAlgoType, HYPRE_Int, s->fs_algo = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAILocalSolveType, HYPRE_Int, s->fs_ls_type = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIMaxSteps, HYPRE_Int, s->fs_max_steps = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIMaxStepSize, HYPRE_Int, s->fs_max_step_size = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIMaxNnzRow, HYPRE_Int, s->fsaip.max_nnz_row = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAINumLevels, HYPRE_Int, s->fsaip.num_levels = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIThreshold, HYPRE_Real, s->fsaip.threshold = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIEigMaxIters, HYPRE_Int, s->fsaip.eig_max_iters = v)
HY_SETTER(HYPRE_BoomerAMGSetFSAIKapTolerance, HYPRE_Real, s->fs_kap_tol = v)

extern "C" HYPRE_Int HYPRE_FSAISetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_TRY
   HDA_REQUIRE(s && is_live_solver(s) && s->kind == HDA_SOLVER_FSAI, "FSAISetup: not an FSAI handle");
   const std::string why = fsai_refusal(s->fs_algo, s->fsaip, s->fs_tol);
   if (!why.empty()) throw Error(why);
   HDA_REQUIRE(Comm::world().size == 1, "FSAI: a world of more than one rank is not implemented (the pattern of a row partition needs off-rank rows of "
                                        "the power of A); one rank with HDA_BLOCKS row blocks is");
   if (!have_device()) throw Error("no HIP device visible: the MI355X solve path has no CPU fallback");
   HDA_REQUIRE(A && A->assembled, "FSAISetup needs an assembled matrix");
   FsaiParams p = s->fsaip;
   // "bj": block Jacobi over the ranks in hypre; on one GPU the row blocks play the ranks (HDA_BLOCKS = V, 0 = the setup's choice), as for ILU
   p.blocks = env_blocks(1);
   s->pc.kind = Precond::FSAI;
   s->pc.fsai = std::make_unique<Fsai>();
   s->pc.fsai->setup(A->A, p);
   const Fsai &F = *s->pc.fsai;
   if (F.nblocks > 1 && !quiet())
      fprintf(stderr, "[hypredrv_amd] FSAI: %d row blocks (HDA_BLOCKS): no pattern leaves its block, as on %d ranks of the reference\n", F.nblocks, F.nblocks);
   if (s->fs_print_level >= 1)
      printf("FSAI (bj-sfsai): num_levels %d, threshold %g, max_nnz_row %d, nnz(G) / n = %.3f, omega = %.6f (%d power steps), fallback rows %d\n", p.num_levels,
             p.threshold, p.max_nnz_row, F.n ? (double)F.factor().nnz / F.n : 0.0, F.omega, p.eig_max_iters, F.fallback_rows);
   hda_register_precond_veclen((size_t)std::max(A->A.ncols, A->A.nrows));
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_FSAISolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return precond_solve(s, A, b, x, false, [&] { HDA_REQUIRE(s && s->pc.fsai, "FSAISolve before FSAISetup"); });
}

// ------------------------------------------------------------------------ AMS
// HYPRE_AMS* as driven by hypredrv_AMSCreate / hypredrv_AMSSetOperators (reference src/internal/ams.c:78-133).  Built (hda_ams.hip,
// DESIGN section 18): the multiplicative cycles 1, 3, 5, 7 with l1-Jacobi smoothing on one rank; ams_refusal names the rest.

static AmsParams ams_params_of(const hypre_Solver_struct *s)
{
   AmsParams p = s->amsp;
   p.alpha     = ams_subspace_amg(s->ams_alpha, p.dimension);
   p.beta      = ams_subspace_amg(s->ams_beta, 1);
   return p;
}
extern "C" HYPRE_Int HYPRE_AMSCreate(HYPRE_Solver *solver)
{
   if (!solver) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_AMSCreate: null output");
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_AMS;
   *solver = s;
   return 0;
}
// (precon.c:138-154 calls this for whatever handle its table holds: NULL is fine, a handle of another kind is not an AMS handle)
extern "C" HYPRE_Int HYPRE_AMSDestroy(HYPRE_Solver s)
{
   if (!s) return 0;
   if (!is_live_solver(s) || s->kind != HDA_SOLVER_AMS) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_AMSDestroy: not an AMS handle");
   return HYPRE_BoomerAMGDestroy(s);
}
HY_SETTER(HYPRE_AMSSetDimension, HYPRE_Int, s->amsp.dimension = v)
HY_SETTER(HYPRE_AMSSetMaxIter, HYPRE_Int, s->amsp.max_iter = v)
HY_SETTER(HYPRE_AMSSetTol, HYPRE_Real, s->amsp.tolerance = v)
HY_SETTER(HYPRE_AMSSetCycleType, HYPRE_Int, s->amsp.cycle_type = v)
HY_SETTER(HYPRE_AMSSetPrintLevel, HYPRE_Int, s->ams_print_level = v)
HY_SETTER(HYPRE_AMSSetAlphaAMGCoarseRelaxType, HYPRE_Int, s->ams_alpha.coarse_relax_type = v)
HY_SETTER(HYPRE_AMSSetBetaAMGCoarseRelaxType, HYPRE_Int, s->ams_beta.coarse_relax_type = v)
HY_SETTER(HYPRE_AMSSetProjectionFrequency, HYPRE_Int, s->ams_proj_freq = v) // (the singular case only)
HY_SETTER(HYPRE_AMSSetDiscreteGradient, HYPRE_ParCSRMatrix, s->ams_G = v)
extern "C" HYPRE_Int HYPRE_AMSSetSmoothingOptions(HYPRE_Solver s, HYPRE_Int relax_type, HYPRE_Int relax_times, HYPRE_Real relax_weight, HYPRE_Real omega)
{
   if (!s) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_AMSSetSmoothingOptions: null solver");
   s->amsp.relax_type = relax_type; s->amsp.relax_times = relax_times; s->amsp.relax_weight = relax_weight;
   s->ams_omega = omega; // (acts with relax_type 2 only)
   return 0;
}
static HYPRE_Int ams_set_amg(HYPRE_Solver s, AmsAmgOptions hypre_Solver_struct::*which, const char *fn, HYPRE_Int coarsen_type, HYPRE_Int agg_levels,
                             HYPRE_Int relax_type, HYPRE_Real theta, HYPRE_Int interp_type, HYPRE_Int pmax)
{
   if (!s) return hypre_set_error(HYPRE_ERROR_ARG, std::string(fn) + ": null solver");
   AmsAmgOptions &o = s->*which;
   o.coarsen_type = coarsen_type; o.agg_levels = agg_levels; o.relax_type = relax_type; o.strength_threshold = theta;
   o.interp_type = interp_type; o.pmax = pmax;
   return 0;
}
extern "C" HYPRE_Int HYPRE_AMSSetAlphaAMGOptions(HYPRE_Solver s, HYPRE_Int coarsen_type, HYPRE_Int agg_levels, HYPRE_Int relax_type,
                                                 HYPRE_Real strength_threshold, HYPRE_Int interp_type, HYPRE_Int Pmax)
{
   return ams_set_amg(s, &hypre_Solver_struct::ams_alpha, "HYPRE_AMSSetAlphaAMGOptions", coarsen_type, agg_levels, relax_type, strength_threshold, interp_type, Pmax);
}
extern "C" HYPRE_Int HYPRE_AMSSetBetaAMGOptions(HYPRE_Solver s, HYPRE_Int coarsen_type, HYPRE_Int agg_levels, HYPRE_Int relax_type,
                                                HYPRE_Real strength_threshold, HYPRE_Int interp_type, HYPRE_Int Pmax)
{
   return ams_set_amg(s, &hypre_Solver_struct::ams_beta, "HYPRE_AMSSetBetaAMGOptions", coarsen_type, agg_levels, relax_type, strength_threshold, interp_type, Pmax);
}
extern "C" HYPRE_Int HYPRE_AMSSetCoordinateVectors(HYPRE_Solver s, HYPRE_ParVector x, HYPRE_ParVector y, HYPRE_ParVector z)
{
   if (!s) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_AMSSetCoordinateVectors: null solver");
   s->ams_xyz[0] = x; s->ams_xyz[1] = y; s->ams_xyz[2] = z;
   return 0;
}

extern "C" HYPRE_Int HYPRE_AMSSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_TRY
   HDA_REQUIRE(s && is_live_solver(s) && s->kind == HDA_SOLVER_AMS, "AMSSetup: not an AMS handle");
   const AmsParams   p   = ams_params_of(s);
   const std::string why = ams_refusal(p);
   if (!why.empty()) throw Error(why);
   HDA_REQUIRE(Comm::world().size == 1, "AMS: a world of more than one rank is not implemented (row partitions of G and Pi are not built); one rank is");
   if (!have_device()) throw Error("no HIP device visible: the MI355X solve path has no CPU fallback");
   HDA_REQUIRE(A && A->assembled, "AMSSetup needs an assembled matrix");
   HYPRE_ParCSRMatrix G = s->ams_G;
   if (!G || !s->ams_xyz[0] || !s->ams_xyz[1] || (p.dimension == 3 && !s->ams_xyz[2]))
      throw Error("AMS setup requires a discrete gradient matrix and coordinate vectors, but they were not provided");
   HDA_REQUIRE(G->assembled, "AMSSetup needs an assembled discrete gradient");
   HDA_REQUIRE(G->A.nrows == A->A.nrows, "AMS: the discrete gradient needs one row per row of the operator");
   HDA_REQUIRE(G->ghost_gids.empty(), "AMS: the discrete gradient names columns outside its column range");
   const double *c[3] = {nullptr, nullptr, nullptr};
   for (int k = 0; k < p.dimension; k++)
   {
      HYPRE_ParVector v = s->ams_xyz[k];
      HDA_REQUIRE(v->nloc == G->A.ncols, "AMS: a coordinate vector needs one entry per column of the discrete gradient");
      v->ensure_device();
      c[k] = v->data();
   }
   s->pc.kind = Precond::AMS;
   s->pc.ams  = std::make_unique<Ams>();
   s->pc.ams->setup(A->A, G->A, c, p);
   Ams &S = *s->pc.ams;
   if (s->ams_print_level >= 1)
      printf("AMS (cycle %d, dimension %d): n_e %d, n_v %d, nnz(Pi) %d, A_G %d rows / %d levels, A_Pi %d rows / %d levels, repaired rows %d + %d\n",
             p.cycle_type, p.dimension, S.n_e, S.n_v, S.pi().nnz, S.a_g().nrows, S.b_g().num_levels(), S.a_pi().nrows, S.b_pi().num_levels(),
             S.fixed_rows[0], S.fixed_rows[1]);
   hda_register_precond_veclen((size_t)std::max(A->A.ncols, A->A.nrows));
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_AMSSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{ // (the cycle is a stationary iteration: from x it gives x + M (b - A x))
   return precond_solve(s, A, b, x, false, [&] {
      HDA_REQUIRE(s && is_live_solver(s) && s->kind == HDA_SOLVER_AMS, "AMSSolve: not an AMS handle");
      HDA_REQUIRE(s->pc.ams, "AMSSolve before AMSSetup");
      HDA_REQUIRE(A && A->assembled && b && x, "AMSSolve needs an assembled matrix and two vectors");
      HDA_REQUIRE(A->A.nrows == s->pc.ams->n_e && b->nloc == A->A.nrows && x->nloc == A->A.nrows, "AMSSolve: the system is not the size of the one set up");
   });
}

// ------------------------------------------------------------------------ MGR
// HYPRE_MGR* as driven by hypredrv_MGRCreate (reference src/internal/mgr.c:3782-3808 base settings, per-level
// arrays after :3820).  hypre's calling convention is kept: C points of every reduction level by dof label
// (SetCpointsByPointMarkerArray), per-level option arrays, a BoomerAMG handle as coarse solver.

extern "C" HYPRE_Int HYPRE_MGRCreate(HYPRE_Solver *solver)
{
   auto *s = new hypre_Solver_struct();
   s->kind = HDA_SOLVER_MGR;
   *solver = s;
   return 0;
}
extern "C" HYPRE_Int HYPRE_MGRDestroy(HYPRE_Solver s) { return HYPRE_BoomerAMGDestroy(s); }
extern "C" HYPRE_Int HYPRE_MGRSetCpointsByPointMarkerArray(HYPRE_Solver s, HYPRE_Int block_size, HYPRE_Int max_num_levels,
                                                           HYPRE_Int *num_block_coarse_points, HYPRE_Int **block_coarse_indexes,
                                                           HYPRE_Int *point_marker_array)
{
   if (!s || max_num_levels < 0 || (max_num_levels > 0 && (!num_block_coarse_points || !block_coarse_indexes)))
      return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_MGRSetCpointsByPointMarkerArray: bad arguments");
   s->mgr_block_size = block_size;
   s->mgr_levels     = max_num_levels;
   s->mgr_marker     = point_marker_array;
   s->mgr_c_labels.assign((size_t)max_num_levels, {});
   for (int l = 0; l < max_num_levels; l++)
      s->mgr_c_labels[(size_t)l].assign(block_coarse_indexes[l], block_coarse_indexes[l] + num_block_coarse_points[l]);
   return 0;
}
#define HY_MGR_LEVEL_ARRAY(fn, member)                                                                       \
   extern "C" HYPRE_Int fn(HYPRE_Solver s, HYPRE_Int *v)                                                      \
   {                                                                                                         \
      if (!s || (!v && s->mgr_levels > 0)) return hypre_set_error(HYPRE_ERROR_ARG, #fn ": null argument");   \
      s->member.assign(v, v + s->mgr_levels);                                                                \
      return 0;                                                                                              \
   }
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelFRelaxType, mgr_frelax)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelNumRelaxSweeps, mgr_fsweeps)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelInterpType, mgr_interp)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelRestrictType, mgr_restrict)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetCoarseGridMethod, mgr_coarse_method)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelSmoothType, mgr_gsmooth)
HY_MGR_LEVEL_ARRAY(HYPRE_MGRSetLevelSmoothIters, mgr_giters)
HY_SETTER(HYPRE_MGRSetNonCpointsToFpoints, HYPRE_Int, (void)v) // every label is either C or F here
HY_SETTER(HYPRE_MGRSetPMaxElmts, HYPRE_Int, (void)v)           // truncation of the classical-modified interpolation only
HY_SETTER(HYPRE_MGRSetNonGalerkinMaxElmts, HYPRE_Int, s->mgr_nonglk_max_elmts = v) // non-Galerkin coarse grids only
HY_SETTER(HYPRE_MGRSetMaxIter, HYPRE_Int, s->mgr_max_iter = v)
HY_SETTER(HYPRE_MGRSetTol, HYPRE_Real, s->ap.tol = v)
HY_SETTER(HYPRE_MGRSetPrintLevel, HYPRE_Int, s->ap.print_level = v)
HY_SETTER(HYPRE_MGRSetCycleType, HYPRE_Int, s->mgr_cycle = v)
HY_SETTER(HYPRE_MGRSetFRelaxCycle, HYPRE_Int, s->mgr_frelax_cycle = v)
HY_SETTER(HYPRE_MGRSetGlobalSmoothCycle, HYPRE_Int, s->mgr_gsmooth_cycle = v)
HY_SETTER(HYPRE_MGRSetTruncateCoarseGridThreshold, HYPRE_Real, s->mgr_coarse_th = v)
HY_SETTER(HYPRE_MGRSetRelaxType, HYPRE_Int, (void)v) // per-level F-relaxation types are given explicitly
extern "C" HYPRE_Int HYPRE_MGRSetCoarseSolver(HYPRE_Solver s, HYPRE_PtrToSolverFcn, HYPRE_PtrToSolverFcn, HYPRE_Solver coarse)
{
   if (!s) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_MGRSetCoarseSolver: null solver");
   s->mgr_csolver = coarse;
   return 0;
}

extern "C" HYPRE_Int HYPRE_MGRSetFSolverAtLevel(HYPRE_Solver s, HYPRE_Solver fsolver, HYPRE_Int level)
{
   if (!s || level < 0 || level > 30) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_MGRSetFSolverAtLevel: bad arguments");
   if ((size_t)level >= s->mgr_fsolver.size()) s->mgr_fsolver.resize((size_t)level + 1, nullptr);
   s->mgr_fsolver[(size_t)level] = fsolver;
   return 0;
}

extern "C" HYPRE_Int HYPRE_MGRSetGlobalSmootherAtLevel(HYPRE_Solver s, HYPRE_Solver smoother, HYPRE_Int level)
{
   if (!s || level < 0 || level > 30) return hypre_set_error(HYPRE_ERROR_ARG, "HYPRE_MGRSetGlobalSmootherAtLevel: bad arguments");
   if ((size_t)level >= s->mgr_gsolver.size()) s->mgr_gsolver.resize((size_t)level + 1, nullptr);
   s->mgr_gsolver[(size_t)level] = smoother;
   return 0;
}

extern "C" HYPRE_Int HYPRE_MGRSetup(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector, HYPRE_ParVector)
{
   HY_NEED_DEVICE;
   HY_TRY
   HDA_REQUIRE(s && s->kind == HDA_SOLVER_MGR, "MGRSetup: not an MGR handle");
   HDA_REQUIRE(A && A->assembled, "MGRSetup needs an assembled matrix");
   HDA_REQUIRE(s->mgr_levels > 0 && s->mgr_marker, "MGRSetup: no C points were set (HYPRE_MGRSetCpointsByPointMarkerArray)");
   HDA_REQUIRE(s->mgr_cycle == 1 || s->mgr_cycle == 2, "MGR cycle type: 1 (V) or 2 (W)");
   HDA_REQUIRE(s->mgr_frelax_cycle >= 1 && s->mgr_frelax_cycle <= 3 && s->mgr_gsmooth_cycle >= 1 && s->mgr_gsmooth_cycle <= 3,
               "MGR smoothing position: 1 (pre), 2 (post) or 3 (both)");
   // a Krylov handle as component solver (the reference's nested Krylov wrapper, src/internal/krylov.c): its parameters and the
   // BoomerAMG / ILU handle installed as its preconditioner
   auto krylov_method = [](HYPRE_Solver q) {
      return !q ? -1 : q->kind == HDA_SOLVER_PCG ? 0 : q->kind == HDA_SOLVER_GMRES ? 1 : q->kind == HDA_SOLVER_FGMRES ? 2 : q->kind == HDA_SOLVER_BICGSTAB ? 3 : -1;
   };
   auto nested = [](HYPRE_Solver q) {
      NestedKrylov k;
      k.max_iter = q->kp.max_iter; k.rtol = q->kp.rtol; k.atol = q->kp.atol; k.krylov_dim = q->kp.krylov_dim; k.min_iter = q->kp.min_iter;
      k.two_norm = q->kp.two_norm; k.skip_real_res_check = q->kp.skip_real_res_check;
      return k;
   };
   auto ilu_ok = [](HYPRE_Solver q) { return q->ilu_type == 0 && q->ilu_fill == 0 && q->ilu_reordering == 0; };
   // component handles come through HYPRE_Solver-typed setters: anything that is not one of this library's live solver objects
   // (a foreign cookie, a destroyed handle) is refused before it is looked into
   auto ours = [](HYPRE_Solver q) { return !q || is_live_solver(q); };
   HDA_REQUIRE(ours(s->mgr_csolver), "MGR coarsest_level: the solver handle is not a live solver object of this library");
   for (HYPRE_Solver q : s->mgr_fsolver) HDA_REQUIRE(ours(q), "MGR f_relaxation: the F-solver handle is not a live solver object of this library");
   for (HYPRE_Solver q : s->mgr_gsolver) HDA_REQUIRE(ours(q), "MGR g_relaxation: the smoother handle is not a live solver object of this library");
   auto precond_of = [&](HYPRE_Solver q) -> HYPRE_Solver { // the preconditioner handle of a Krylov component
      HDA_REQUIRE(ours(q->precond_solver), "MGR: the preconditioner of a nested Krylov solver is not a live solver object of this library");
      return q->precond_solver;
   };
   MgrParams    p;
   HYPRE_Solver cs = s->mgr_csolver;
   if (krylov_method(cs) >= 0)
   {
      p.ckrylov_method  = krylov_method(cs);
      p.ckrylov         = nested(cs);
      p.ckrylov_precond = precond_of(cs) != nullptr;
      cs                = precond_of(cs); // what preconditions it; none: the coarse hierarchy below is built and left unused
   }
   HDA_REQUIRE(!cs || cs->kind == HDA_SOLVER_AMG || cs->kind == HDA_SOLVER_ILU,
               "MGR coarsest_level: BoomerAMG, ILU and a Krylov solver preconditioned by one of them are implemented");
   p.max_iter = s->mgr_max_iter;
   p.cycle = s->mgr_cycle; p.frelax_pos = s->mgr_frelax_cycle; p.gsmooth_pos = s->mgr_gsmooth_cycle;
   if (cs && cs->kind == HDA_SOLVER_ILU)
   {
      HDA_REQUIRE(ilu_ok(cs), "MGR coarsest_level ilu: only type bj-iluk with fill_level 0 and reordering 0 is implemented");
      p.coarse_is_ilu = true;
      p.coarse_ilu    = cs->ilup;
   }
   else if (cs) p.coarse = cs->ap;
   else { AmgParams d; p.coarse = d; }
   p.coarse.max_iter = 1; // one V-cycle per MGR cycle (amg.c:224-226 defaults)
   // F labels of level l = C labels of level l-1 (all labels of the marker array for l = 0) that are no longer C
   std::vector<int> labels(s->mgr_marker, s->mgr_marker + A->nloc);
   std::vector<int> prev;
   {
      std::vector<int> seen = labels;
      std::sort(seen.begin(), seen.end());
      seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
      prev = seen;
   }
   auto at = [&](const std::vector<int> &v, int l, int dflt) { return (size_t)l < v.size() ? v[(size_t)l] : dflt; };
   for (int l = 0; l < s->mgr_levels; l++)
   {
      MgrLevelParams   q;
      std::vector<int> c = s->mgr_c_labels[(size_t)l];
      std::sort(c.begin(), c.end());
      for (int lab : prev)
         if (!std::binary_search(c.begin(), c.end(), lab)) q.f_labels.push_back(lab);
      q.interp_type   = at(s->mgr_interp, l, 0);
      q.restrict_type = at(s->mgr_restrict, l, 0);
      q.coarse_type   = at(s->mgr_coarse_method, l, 0);
      q.nonglk_max_elmts = s->mgr_nonglk_max_elmts;
      q.coarse_th        = s->mgr_coarse_th;
      q.frelax_type   = at(s->mgr_frelax, l, 7);
      {
         HYPRE_Solver fk = (size_t)l < s->mgr_fsolver.size() ? s->mgr_fsolver[(size_t)l] : nullptr;
         if (krylov_method(fk) >= 0)
         { // F-relaxation by a nested Krylov solve: the component underneath is its preconditioner (BoomerAMG when there is none to name)
            q.fkrylov_method  = krylov_method(fk);
            q.fkrylov         = nested(fk);
            HYPRE_Solver fp   = precond_of(fk);
            q.fkrylov_precond = fp != nullptr;
            HDA_REQUIRE(!fp || fp->kind == HDA_SOLVER_AMG || fp->kind == HDA_SOLVER_ILU,
                        "MGR f_relaxation: a nested Krylov solver takes BoomerAMG, ILU or no preconditioner");
            q.frelax_type = (fp && fp->kind == HDA_SOLVER_ILU) ? 32 : 2;
         }
      }
      if (q.frelax_type == 2 || q.frelax_type == 32)
      {
         HYPRE_Solver fs = (size_t)l < s->mgr_fsolver.size() ? s->mgr_fsolver[(size_t)l] : nullptr;
         if (krylov_method(fs) >= 0) fs = precond_of(fs);
         HDA_REQUIRE(!fs || fs->kind == (q.frelax_type == 2 ? HDA_SOLVER_AMG : HDA_SOLVER_ILU), "MGR f_relaxation: the F-solver handle does not match its type (amg / ilu)");
         if (fs && q.frelax_type == 2)
         {
            HDA_REQUIRE(fs->filter_functions == 0 || fs->num_functions <= 1, "coarsening.filter_functions is not implemented for systems AMG");
            q.frelax_amg = fs->ap; q.frelax_amg.num_functions = std::max(fs->num_functions, 1);
         }
         if (fs && q.frelax_type == 32)
         {
            HDA_REQUIRE(ilu_ok(fs), "MGR f_relaxation ilu: only type bj-iluk with fill_level 0 and reordering 0 is implemented");
            q.ilu = fs->ilup;
         }
      }
      q.frelax_sweeps = at(s->mgr_fsweeps, l, 1);
      q.grelax_type   = at(s->mgr_gsmooth, l, -1);
      q.grelax_sweeps = at(s->mgr_giters, l, 1);
      if (q.grelax_sweeps <= 0) q.grelax_type = -1; // hypre: no global smoothing without sweeps
      // row blocks of a hybrid Gauss-Seidel global relaxation, as for BoomerAMG's sweeps: HDA_BLOCKS = V, 1 = one block (np = 1), unset = the
      // setup's choice (one block up to 100 000 rows; announced); across ranks the rank blocks are the blocks
      q.grelax_blocks = (Comm::world().size > 1) ? 1 : env_blocks(0);
      if ((size_t)l < s->mgr_gsolver.size() && s->mgr_gsolver[(size_t)l])
      { // a smoother object handed over with HYPRE_MGRSetGlobalSmootherAtLevel (mgr.c: ILU with its own arguments)
         HYPRE_Solver gs = s->mgr_gsolver[(size_t)l];
         HDA_REQUIRE(gs->kind == HDA_SOLVER_ILU && ilu_ok(gs), "MGR g_relaxation: only an ILU (bj-iluk, fill_level 0, reordering 0) smoother object is implemented");
         q.grelax_type   = 16;
         q.grelax_sweeps = std::max(q.grelax_sweeps, 1);
         const IluParams keep = q.frelax_type == 32 ? q.ilu : gs->ilup;
         q.ilu           = keep; // (one set of ILU arguments per level: the F-solver's wins when both are ILU)
      }
      p.levels.push_back(q);
      prev = c;
   }
   s->pc.kind = Precond::MGR;
   s->pc.mgr  = std::make_unique<Mgr>(p);
   if (Comm::world().size > 1) s->pc.mgr->setup_dist(A->A, A->halo, A->part, A->ghost_gids, labels);
   else s->pc.mgr->setup(A->A, labels);
   hda_register_precond_veclen(s->pc.mgr->vec_len0());
   if (s->ap.print_level > 0)
   { // the reduction hierarchy (global sizes), in the spirit of hypre's MGR setup printout
      const int nl = s->pc.mgr->num_reduction_levels();
      std::vector<long long> sz((size_t)(2 * (nl + 1)));
      for (int l = 0; l <= nl; l++)
      {
         const DCsr &M        = s->pc.mgr->matrix(l, 0);
         sz[(size_t)(2 * l)]     = M.nrows;
         sz[(size_t)(2 * l + 1)] = M.nnz;
      }
      Comm::world().allreduce_host(sz.data(), (int)sz.size(), 0);
      if (Comm::world().rank == 0)
      {
         printf("\n MGR (MI355X): %d reduction level%s + coarsest system\n   lev        rows     nonzeros   eliminated labels\n", nl, nl == 1 ? "" : "s");
         for (int l = 0; l <= nl; l++)
         {
            printf("   %3d  %10lld  %11lld   ", l, sz[(size_t)(2 * l)], sz[(size_t)(2 * l + 1)]);
            if (l < nl)
               for (int f : p.levels[(size_t)l].f_labels) printf("%d ", f);
            else printf("(%s)", p.coarse_is_ilu ? "ILU" : "BoomerAMG");
            printf("\n");
         }
         printf("\n");
      }
   }
   HY_CATCH
}

extern "C" HYPRE_Int HYPRE_MGRSolve(HYPRE_Solver s, HYPRE_ParCSRMatrix A, HYPRE_ParVector b, HYPRE_ParVector x)
{
   return precond_solve(s, A, b, x, true, [&] {
      HDA_REQUIRE(s && s->pc.mgr, "MGRSolve before MGRSetup");
      if (!s->pc.mgr->bound_to(A->A)) s->pc.mgr->rebind(A->A, Comm::world().size > 1 ? &A->halo : nullptr); // reused preconditioner, later system
   });
}
HY_GETTER(HYPRE_MGRGetNumIterations, HYPRE_Int, s->amg_iters)
HY_GETTER(HYPRE_MGRGetFinalRelativeResidualNorm, HYPRE_Real, s->amg_rel)

HY_GETTER(HYPRE_BoomerAMGGetNumIterations, HYPRE_Int, s->amg_iters)
HY_GETTER(HYPRE_BoomerAMGGetFinalRelativeResidualNorm, HYPRE_Real, s->amg_rel)
HY_GETTER(HYPRE_BoomerAMGGetNumLevels, HYPRE_Int, s->pc.amg ? s->pc.amg->num_levels() : 0)
extern "C" HYPRE_Int HYPRE_BoomerAMGGetComplexities(HYPRE_Solver s, HYPRE_Real *grid, HYPRE_Real *op)
{
   if (!s || !s->pc.amg) return hypre_set_error(HYPRE_ERROR_ARG, "GetComplexities before Setup");
   if (grid) *grid = s->pc.amg->grid_complexity();
   if (op) *op = s->pc.amg->operator_complexity();
   return 0;
}

// ------------------------------------------------------------------ the rest of the lower seam (round 5)
// Every HYPRE_* name the reference files of SURVEY 8(a) call (src/internal/{amg,pcg,gmres,ilu,solver,precon}.c) resolves in this
// library, so an unmodified libHYPREDRV links against it as it is (tests/test_cabi_symbols.py::test_lower_seam_names_resolve,
// names in tests/golden/hypre_lower_seam_names.txt).  What is outside SURVEY 8 is REFUSED BY NAME: the call sets hypre's error
// flag with a message and returns non-zero -- never ignored.  (The FSAI parameter setters, which amg.c:924-932 calls for EVERY BoomerAMG
// whatever its smoother, record their values: the FSAI section above.)

#define HY_REFUSED(fn, args, what) \
   extern "C" HYPRE_Int fn args { return hypre_set_error(HYPRE_ERROR_GENERIC, #fn ": " what " is not part of the MI355X solve path (SURVEY 8: out of scope)"); }
// coarsening.nodal with rigid-body-mode interpolation vectors (amg.c:1017-1032)
HY_REFUSED(HYPRE_BoomerAMGSetNodal, (HYPRE_Solver, HYPRE_Int), "nodal coarsening")
HY_REFUSED(HYPRE_BoomerAMGSetNodalDiag, (HYPRE_Solver, HYPRE_Int), "nodal coarsening")
HY_REFUSED(HYPRE_BoomerAMGSetInterpVecVariant, (HYPRE_Solver, HYPRE_Int), "interpolation with near-null-space vectors")
HY_REFUSED(HYPRE_BoomerAMGSetInterpVecQMax, (HYPRE_Solver, HYPRE_Int), "interpolation with near-null-space vectors")
HY_REFUSED(HYPRE_BoomerAMGSetSmoothInterpVectors, (HYPRE_Solver, HYPRE_Int), "interpolation with near-null-space vectors")
HY_REFUSED(HYPRE_BoomerAMGSetInterpVectors, (HYPRE_Solver, HYPRE_Int, HYPRE_ParVector *), "interpolation with near-null-space vectors")
// error tracking against a reference solution inside GMRES (gmres.c:86-98)
HY_REFUSED(HYPRE_ParCSRGMRESSetRefSolution, (HYPRE_Solver, HYPRE_ParVector), "error tracking against a reference solution")
#undef HY_REFUSED
// destroy entries of precon_ops for preconditioners that cannot have been created here (precon.c:138-154): NULL is fine, anything else
// is not a handle of this library
#define HY_FOREIGN_DESTROY(fn, what) \
   extern "C" HYPRE_Int fn(HYPRE_Solver s) { return s ? hypre_set_error(HYPRE_ERROR_ARG, #fn ": " what " handles are never created by this library") : 0; }
HY_FOREIGN_DESTROY(HYPRE_ADSDestroy, "ADS")
#undef HY_FOREIGN_DESTROY

// HYPRE_ParVector{Create,Initialize,Destroy} (amg.c:557, precon.c:770-783): a ParVector IS this library's IJ vector (HYPRE.h);
// partitioning = {first row, one past the last row} of the calling rank, NULL = hypre's even split of global_size over the ranks
extern "C" HYPRE_Int HYPRE_ParVectorCreate(MPI_Comm comm, HYPRE_BigInt global_size, HYPRE_BigInt *partitioning, HYPRE_ParVector *vector)
{
   HY_TRY
   HDA_REQUIRE(vector, "HYPRE_ParVectorCreate: null output");
   mpi_autojoin((int)comm);
   const Comm &cm = Comm::world();
   long long lo, hi;
   if (partitioning) { lo = partitioning[0]; hi = partitioning[1]; }
   else
   { // hypre_GeneratePartitioning: size / ranks each, the first (size % ranks) ranks one more
      const long long q = global_size / cm.size, r = global_size % cm.size;
      lo = cm.rank * q + std::min<long long>(cm.rank, r);
      hi = lo + q + (cm.rank < r ? 1 : 0);
   }
   return HYPRE_IJVectorCreate(comm, lo, hi - 1, vector);
   HY_CATCH
}
extern "C" HYPRE_Int HYPRE_ParVectorInitialize(HYPRE_ParVector v) { return HYPRE_IJVectorInitialize(v); }
extern "C" HYPRE_Int HYPRE_ParVectorDestroy(HYPRE_ParVector v) { return HYPRE_IJVectorDestroy(v); }
