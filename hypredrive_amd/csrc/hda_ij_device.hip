// hda_ij_device.hip -- the IJ interface for callers whose arrays live in HBM (HYPRE_IJMatrixInitialize_v2 / HYPRE_IJVectorInitialize_v2
// with HYPRE_MEMORY_DEVICE).  Matrix calls go onto a device-side stack in call order and HYPRE_IJMatrixAssemble builds
// the operator from it on the device; vector calls are applied to the vector's HBM storage at once.  What comes out is defined by the
// host path (hypre_IJMatrix_struct::assemble, vec_set in hda_hypre.hip) and is bit for bit what that path builds from the same calls:
// per (row, column) the contributions are taken in call order, the first as it is, a later set replaces, a later add does
// value = value + v.  No float atomics: equal keys are brought together by one STABLE sort and every run is summed by one thread.
#include "hda_hypre.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

using namespace hda;

#define STREAM (Context::get().stream)

namespace {

constexpr unsigned long long kNone = ~0ull;

inline int grid_for(long long n) { return std::max(1, std::min(ceil_div(n, 256), 1 << 16)); }
inline int bits_for(long long n) // bits that hold every value of [0, n)
{
   int b = 1;
   while (b < 63 && (1LL << b) < n) b++;
   return b;
}

// ---- matrix stack

__global__ __launch_bounds__(256) void k_ij_counts(int nrows, const int *__restrict__ ncols, long long *__restrict__ cnt)
{
   const int r = blockIdx.x * 256 + threadIdx.x;
   if (r < nrows) cnt[r] = ncols[r] > 0 ? ncols[r] : 0;
   else if (r == nrows) cnt[r] = 0;
}

// One launch per SetValues / AddToValues call.  Rows: the first entry position of the first row outside [ilower, ilower + nloc) goes to
// *first_bad (the host path stacks what precedes that row and then refuses the call).  Entries: entry e of the call belongs to the last
// row r with offs[r] <= e (rows without columns share their offset with the next one); its local row id, global column, value and flag
// are written behind the stack, coalesced whatever the row lengths.
__global__ __launch_bounds__(256) void k_ij_expand(int nrows, long long T, const long long *__restrict__ offs, const long long *__restrict__ rows,
                                                   const long long *__restrict__ cols, const double *__restrict__ vals, long long ilower, int nloc,
                                                   unsigned char flag, int *__restrict__ orow, long long *__restrict__ ocol, double *__restrict__ oval,
                                                   unsigned char *__restrict__ oadd, unsigned long long *first_bad)
{
   const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
   for (long long r = t0; r < nrows; r += stride)
   {
      const long long l = rows[r] - ilower;
      if (l < 0 || l >= nloc) atomicMin(first_bad, (unsigned long long)offs[r]);
   }
   for (long long e = t0; e < T; e += stride)
   {
      int lo = 0, hi = nrows - 1;
      while (lo < hi)
      {
         const int mid = (int)(((long long)lo + hi + 1) >> 1);
         if (offs[mid] <= e) lo = mid;
         else hi = mid - 1;
      }
      orow[e] = (int)(rows[lo] - ilower);
      ocol[e] = cols[e];
      oval[e] = vals[e];
      oadd[e] = flag;
   }
}

// every entry a set and the row ids never decreasing: the stack is a CSR block already
__global__ __launch_bounds__(256) void k_ij_stack_is_csr(long long T, const int *__restrict__ row, const unsigned char *__restrict__ add, int *not_csr)
{
   for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < T; e += (long long)gridDim.x * 256)
      if (add[e] || (e > 0 && row[e] < row[e - 1])) *not_csr = 1;
}
// indptr of such a stack: ip[i] = entries in rows < i
__global__ __launch_bounds__(256) void k_ij_indptr(int nloc, long long T, const int *__restrict__ row, long long *__restrict__ ip)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i > nloc) return;
   long long lo = 0, hi = T;
   while (lo < hi)
   {
      const long long mid = (lo + hi) >> 1;
      if (row[mid] < i) lo = mid + 1;
      else hi = mid;
   }
   ip[i] = lo;
}

__global__ __launch_bounds__(256) void k_ij_keys(long long T, const int *__restrict__ row, const int *__restrict__ lcol, unsigned long long *__restrict__ key,
                                                 unsigned int *__restrict__ pos)
{
   for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < T; e += (long long)gridDim.x * 256)
   {
      key[e] = ((unsigned long long)(unsigned int)row[e] << 32) | (unsigned int)lcol[e];
      pos[e] = (unsigned int)e;
   }
}
__global__ __launch_bounds__(256) void k_ij_heads(long long T, const unsigned long long *__restrict__ key, int *__restrict__ head)
{
   for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < T; e += (long long)gridDim.x * 256) head[e] = (e == 0 || key[e] != key[e - 1]) ? 1 : 0;
}
// rid: the inclusive scan of head.  start[r] = first sorted position of run r, start[nruns] = T
__global__ __launch_bounds__(256) void k_ij_run_starts(long long T, const unsigned long long *__restrict__ key, const int *__restrict__ rid, int *__restrict__ start)
{
   for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < T; e += (long long)gridDim.x * 256)
   {
      if (e == 0 || key[e] != key[e - 1]) start[rid[e] - 1] = (int)e;
      if (e == T - 1) start[rid[e]] = (int)T;
   }
}
// One thread per run of equal (row, column): its contributions in ascending stack position (the sort is stable), the first as it is, a
// set replaces, an add accumulates left to right.  Run r is entry r of the CSR block; the thread also writes the row pointers of the rows
// that start at r (its own row when the previous run lies in an earlier one, and the empty rows in between).
__global__ __launch_bounds__(256) void k_ij_reduce_runs(int nruns, int nloc, const int *__restrict__ start, const unsigned long long *__restrict__ key,
                                                        const unsigned int *__restrict__ pos, const double *__restrict__ val,
                                                        const unsigned char *__restrict__ add, int *__restrict__ rowptr, int *__restrict__ col,
                                                        double *__restrict__ out)
{
   const int r = blockIdx.x * 256 + threadIdx.x;
   if (r >= nruns) return;
   const int                s = start[r], e = start[r + 1];
   const unsigned long long k = key[s];
   unsigned int             p = pos[s];
   double                   acc = val[p];
   for (int j = s + 1; j < e; j++)
   {
      p              = pos[j];
      const double x = val[p];
      acc            = add[p] ? acc + x : x;
   }
   col[r] = (int)(unsigned int)(k & 0xffffffffull);
   out[r] = acc;
   const int row = (int)(k >> 32), prev = r ? (int)(key[s - 1] >> 32) : -1;
   for (int i = prev + 1; i <= row; i++) rowptr[i] = r;
   if (r == nruns - 1)
      for (int i = row + 1; i <= nloc; i++) rowptr[i] = nruns;
}

// ---- vectors

__global__ __launch_bounds__(256) void k_vec_stream(int n, const double *__restrict__ val, double *__restrict__ x, int add)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) x[q] = add ? x[q] + val[q] : val[q];
}
// chk[0]: first position whose index leaves the local range; chk[1]: != 0 when the indices are not strictly increasing
__global__ __launch_bounds__(256) void k_vec_check(int n, const long long *__restrict__ idx, long long jlower, int nloc, unsigned long long *chk)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256)
   {
      const long long l = idx[q] - jlower;
      if (l < 0 || l >= nloc) atomicMin(&chk[0], (unsigned long long)q);
      if (q > 0 && idx[q] <= idx[q - 1]) chk[1] = 1;
   }
}
// strictly increasing indices: every destination is named once
__global__ __launch_bounds__(256) void k_vec_scatter(int n, const long long *__restrict__ idx, long long jlower, const double *__restrict__ val,
                                                     double *__restrict__ x, int add)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256)
   {
      const long long l = idx[q] - jlower;
      x[l]              = add ? x[l] + val[q] : val[q];
   }
}
__global__ __launch_bounds__(256) void k_vec_keys(int n, const long long *__restrict__ idx, long long jlower, unsigned int *__restrict__ key, unsigned int *__restrict__ pos)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256)
   {
      key[q] = (unsigned int)(idx[q] - jlower);
      pos[q] = (unsigned int)q;
   }
}
// sorted (stable) by destination: the thread at the head of a run applies the run in index-array order -- adds one after the other onto
// what the vector holds, of sets the last
__global__ __launch_bounds__(256) void k_vec_reduce_runs(int n, const unsigned int *__restrict__ key, const unsigned int *__restrict__ pos,
                                                         const double *__restrict__ val, double *__restrict__ x, int add)
{
   for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256)
   {
      const unsigned int l = key[j];
      if (j > 0 && key[j - 1] == l) continue;
      double acc = add ? x[l] + val[pos[j]] : val[pos[j]];
      for (long long t = j + 1; t < n && key[t] == l; t++) acc = add ? acc + val[pos[t]] : val[pos[t]];
      x[l] = acc;
   }
}
__global__ __launch_bounds__(256) void k_vec_check_range(int n, const long long *__restrict__ idx, long long jlower, int nloc, unsigned long long *chk)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256)
   {
      const long long l = idx[q] - jlower;
      if (l < 0 || l >= nloc) atomicMin(&chk[0], (unsigned long long)q);
   }
}
__global__ __launch_bounds__(256) void k_vec_gather(int n, const long long *__restrict__ idx, long long jlower, const double *__restrict__ x, double *__restrict__ out)
{
   for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) out[q] = x[idx ? idx[q] - jlower : q];
}

} // namespace

// ------------------------------------------------------------------- the stack

void IjStack::reserve(size_t need)
{
   if (need <= row.size()) return;
   const size_t cap = std::max(need, 2 * row.size());
   DArray<int>           r(cap);
   DArray<long long>     c(cap);
   DArray<double>        v(cap);
   DArray<unsigned char> a(cap);
   if (size)
   {
      HDA_HIP(hipMemcpyAsync(r.data(), row.data(), sizeof(int) * size, hipMemcpyDeviceToDevice, STREAM));
      HDA_HIP(hipMemcpyAsync(c.data(), col.data(), sizeof(long long) * size, hipMemcpyDeviceToDevice, STREAM));
      HDA_HIP(hipMemcpyAsync(v.data(), val.data(), sizeof(double) * size, hipMemcpyDeviceToDevice, STREAM));
      HDA_HIP(hipMemcpyAsync(a.data(), add.data(), size, hipMemcpyDeviceToDevice, STREAM));
   }
   row = std::move(r);
   col = std::move(c);
   val = std::move(v);
   add = std::move(a);
}
void IjStack::clear()
{
   row.release();
   col.release();
   val.release();
   add.release();
   size = 0;
}

bool hda::ij_matrix_push_device(hypre_IJMatrix_struct *m, int nrows, const int *ncols, const long long *rows, const long long *cols,
                                const double *vals, bool add)
{
   if (nrows <= 0) return true;
   // where every row's entries start in the call's cols / values: exclusive scan of the (non-negative) row lengths, the total behind it
   DArray<long long> cnt((size_t)nrows + 1), offs((size_t)nrows + 1);
   k_ij_counts<<<ceil_div((long long)nrows + 1, 256), 256, 0, STREAM>>>(nrows, ncols, cnt.data());
   size_t tmp_bytes = 0;
   HDA_ROCPRIM(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt.data(), offs.data(), 0LL, (size_t)nrows + 1, rocprim::plus<long long>(), STREAM));
   DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
   HDA_ROCPRIM(rocprim::exclusive_scan(tmp.data(), tmp_bytes, cnt.data(), offs.data(), 0LL, (size_t)nrows + 1, rocprim::plus<long long>(), STREAM));
   long long T = 0;
   download_sync(&T, offs.data() + nrows, sizeof(long long));
   HDA_REQUIRE((unsigned long long)T + m->stack.size < (1ULL << 31), "the stacked IJMatrix entries must fit int32");
   IjStack &st = m->stack;
   st.reserve(st.size + (size_t)T);
   DArray<unsigned long long> bad(1);
   HDA_HIP(hipMemsetAsync(bad.data(), 0xff, sizeof(unsigned long long), STREAM));
   const size_t o = st.size;
   k_ij_expand<<<grid_for(std::max<long long>(T, nrows)), 256, 0, STREAM>>>(nrows, T, offs.data(), rows, cols, vals, m->ilower, m->nloc, add ? 1 : 0,
                                                                            st.row.data() + o, st.col.data() + o, st.val.data() + o, st.add.data() + o,
                                                                            bad.data());
   unsigned long long first_bad = kNone;
   bad.download(&first_bad, 1); // (the stream is drained here: the caller's arrays have been read)
   if (first_bad != kNone)
   {
      st.size += (size_t)first_bad;
      return false;
   }
   st.size += (size_t)T;
   return true;
}

// ------------------------------------------------------------------- Assemble

IjAssemblyStats &hda::ij_assembly_stats() { return RankState<IjAssemblyStats>::get(); }

namespace {
// stream time between two points of the general path (tools/side_configs.py assemble quotes the sort and the run reduction)
struct Stamp {
   hipEvent_t e = nullptr;
   Stamp() { HDA_HIP(hipEventCreate(&e)); }
   ~Stamp() { (void)hipEventDestroy(e); }
   void mark() { HDA_HIP(hipEventRecord(e, STREAM)); }
   double ms_since(const Stamp &a) const
   {
      float ms = 0.f;
      HDA_HIP(hipEventElapsedTime(&ms, a.e, e));
      return ms;
   }
};
} // namespace

void hypre_IJMatrix_struct::assemble_device()
{
   const size_t T = stack.size;
   IjAssemblyStats &stats = ij_assembly_stats();
   stats = IjAssemblyStats();
   stats.stacked = (long long)T;
   HDA_REQUIRE(T < (1ULL << 31), "the stacked IJMatrix entries must fit int32");
   if (T == 0)
   { // nothing was set: the empty block of the host path
      DArray<int>       drp((size_t)nloc + 1);
      DArray<long long> dgc(1);
      DArray<double>    dv(1);
      drp.zero();
      ghost_gids.clear();
      adopt_device(nloc, 0, drp, dgc, dv);
      stack.clear();
      return;
   }
   // Set-only calls with rows in order are a CSR block already (the host path's test, assemble() in hda_hypre.hip): build its indptr and
   // go where HYPREDRV_LinearSystemSetMatrixFromCSR goes after its uploads.  A row that names a column twice comes back and takes the
   // general path below, as on the host.
   if (!(getenv("HDA_CSR_DIRECT") && atoi(getenv("HDA_CSR_DIRECT")) == 0))
   {
      DArray<int> flag(1);
      flag.zero();
      k_ij_stack_is_csr<<<grid_for((long long)T), 256, 0, STREAM>>>((long long)T, stack.row.data(), stack.add.data(), flag.data());
      int not_csr = 0;
      flag.download(&not_csr, 1);
      if (!not_csr)
      {
         DArray<long long> dip((size_t)nloc + 1);
         DArray<double>    dv(T);
         k_ij_indptr<<<ceil_div((long long)nloc + 1, 256), 256, 0, STREAM>>>(nloc, (long long)T, stack.row.data(), dip.data());
         HDA_HIP(hipMemcpyAsync(dv.data(), stack.val.data(), sizeof(double) * T, hipMemcpyDeviceToDevice, STREAM)); // (the stack survives a refusal)
         if (assemble_csr_device(dip, stack.col, dv, (long long)T))
         {
            stats.path   = 1;
            stats.merged = A.nnz;
            stack.clear();
            return;
         }
      }
   }
   // General path: (row, local column) keys with the stack position as payload, one stable sort, runs reduced in stack order
   Stamp t[4];
   collect_ghosts(stack.col.data(), (long long)T);
   const int g = grid_for((long long)T);
   DArray<unsigned long long> skey(T);
   DArray<unsigned int>       spos(T);
   {
      DArray<int> lcol(T);
      map_columns(stack.col.data(), (long long)T, lcol.data());
      DArray<unsigned long long> key(T);
      DArray<unsigned int>       pos(T);
      k_ij_keys<<<g, 256, 0, STREAM>>>((long long)T, stack.row.data(), lcol.data(), key.data(), pos.data());
      const unsigned end_bit   = (unsigned)(32 + bits_for(nloc));
      size_t         tmp_bytes = 0;
      HDA_ROCPRIM(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.data(), skey.data(), pos.data(), spos.data(), T, 0, end_bit, STREAM));
      DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
      t[0].mark();
      HDA_ROCPRIM(rocprim::radix_sort_pairs(tmp.data(), tmp_bytes, key.data(), skey.data(), pos.data(), spos.data(), T, 0, end_bit, STREAM));
      t[1].mark();
   }
   int         nruns = 0;
   DArray<int> start;
   {
      DArray<int> head(T), rid(T);
      k_ij_heads<<<g, 256, 0, STREAM>>>((long long)T, skey.data(), head.data());
      size_t tmp_bytes = 0;
      HDA_ROCPRIM(rocprim::inclusive_scan(nullptr, tmp_bytes, head.data(), rid.data(), T, rocprim::plus<int>(), STREAM));
      DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
      HDA_ROCPRIM(rocprim::inclusive_scan(tmp.data(), tmp_bytes, head.data(), rid.data(), T, rocprim::plus<int>(), STREAM));
      download_sync(&nruns, rid.data() + (T - 1), sizeof(int));
      start.alloc((size_t)nruns + 1);
      k_ij_run_starts<<<g, 256, 0, STREAM>>>((long long)T, skey.data(), rid.data(), start.data());
   }
   A       = DCsr();
   A.nrows = nloc;
   A.nnz   = nruns;
   A.ncols = (int)(jupper - jlower + 1) + (int)ghost_gids.size();
   A.rowptr.alloc((size_t)nloc + 1);
   A.col.alloc((size_t)nruns);
   A.val.alloc((size_t)nruns);
   t[2].mark();
   k_ij_reduce_runs<<<ceil_div(nruns, 256), 256, 0, STREAM>>>(nruns, nloc, start.data(), skey.data(), spos.data(), stack.val.data(), stack.add.data(),
                                                              A.rowptr.data(), A.col.data(), A.val.data());
   t[3].mark();
   finish_assembly(); // (rows are sorted and merged: no row sort, no duplicate check)
   stats.path      = 2;
   stats.merged    = nruns;
   stats.sort_ms   = t[1].ms_since(t[0]);
   stats.reduce_ms = t[3].ms_since(t[2]);
   stack.clear();
}

// -------------------------------------------------------------------- vectors

bool hda::ij_vector_set_device(hypre_IJVector_struct *v, int n, const long long *idx, const double *val, bool add)
{
   if (n <= 0) return true;
   v->ensure_device();
   double *x  = v->data(); // (bumps the version counter)
   int     ne = n;         // entries in front of the first index outside the local range: applied, as on the host
   if (!idx)
   {
      ne = std::min(n, v->nloc);
      if (ne > 0) k_vec_stream<<<grid_for(ne), 256, 0, STREAM>>>(ne, val, x, add ? 1 : 0);
      Context::get().sync();
      return ne == n;
   }
   DArray<unsigned long long> chk(2);
   const unsigned long long   init[2] = {kNone, 0};
   chk.upload(init, 2);
   k_vec_check<<<grid_for(n), 256, 0, STREAM>>>(n, idx, v->jlower, v->nloc, chk.data());
   unsigned long long got[2] = {kNone, 0};
   chk.download(got, 2);
   if (got[0] != kNone) ne = (int)got[0];
   if (ne > 0 && !got[1]) k_vec_scatter<<<grid_for(ne), 256, 0, STREAM>>>(ne, idx, v->jlower, val, x, add ? 1 : 0);
   else if (ne > 0)
   { // an index may be named more than once: positions sorted by destination (stable), every run applied in index-array order
      DArray<unsigned int> key((size_t)ne), pos((size_t)ne), skey((size_t)ne), spos((size_t)ne);
      k_vec_keys<<<grid_for(ne), 256, 0, STREAM>>>(ne, idx, v->jlower, key.data(), pos.data());
      const unsigned end_bit   = (unsigned)std::min(bits_for(v->nloc), 32);
      size_t         tmp_bytes = 0;
      HDA_ROCPRIM(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.data(), skey.data(), pos.data(), spos.data(), (size_t)ne, 0, end_bit, STREAM));
      DArray<char> tmp(std::max<size_t>(tmp_bytes, 1));
      HDA_ROCPRIM(rocprim::radix_sort_pairs(tmp.data(), tmp_bytes, key.data(), skey.data(), pos.data(), spos.data(), (size_t)ne, 0, end_bit, STREAM));
      k_vec_reduce_runs<<<grid_for(ne), 256, 0, STREAM>>>(ne, skey.data(), spos.data(), val, x, add ? 1 : 0);
   }
   Context::get().sync();
   return ne == n;
}

bool hda::ij_vector_get_device(hypre_IJVector_struct *v, int n, const long long *idx, double *out)
{
   if (n <= 0) return true;
   v->ensure_device();
   int ne = n;
   if (!idx) ne = std::min(n, v->nloc);
   else
   {
      DArray<unsigned long long> chk(1);
      HDA_HIP(hipMemsetAsync(chk.data(), 0xff, sizeof(unsigned long long), STREAM));
      k_vec_check_range<<<grid_for(n), 256, 0, STREAM>>>(n, idx, v->jlower, v->nloc, chk.data());
      unsigned long long got = kNone;
      chk.download(&got, 1);
      if (got != kNone) ne = (int)got;
   }
   if (ne > 0) k_vec_gather<<<grid_for(ne), 256, 0, STREAM>>>(ne, idx, v->jlower, v->cdata(), out);
   Context::get().sync();
   return ne == n;
}
