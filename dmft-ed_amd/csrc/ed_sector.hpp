// ed_sector.hpp — internal header of the library's host translation units
// over the sector object (ed_lib.hip: life cycle and process-wide state;
// ed_build.hip: the H builders; ed_hxv.hip: the H·v launchers; ed_lanczos.hip:
// the Lanczos drivers; ed_eigh.hip: the thick-restart eigensolver): the
// sector object, its stream-ordered allocator, the per-launch predicates
// asked on every step (static inline here, in namespace edg), and the
// declarations of the functions that cross a unit boundary.
// Process-wide state (the error slot, the pinned pool, the resident_grid
// cache, the singleton API's globals) is defined once, in ed_lib.hip, and
// reached through the functions declared here and in ed_host.hpp.
//
// Sector object = what the reference keeps in module state between
// build_Hv_sector and delete_Hv_sector (ED_HAMILTONIAN_SHARED.f90:32-34,
// ED_VARS_GLOBAL.f90:104-105): the basis H%map, the stored H spH0 (here a
// device SELL-64 matrix) or the matrix-free kernel's tables, plus the
// device-resident Lanczos workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ed_kernels.hpp"
#include "ed_fused.hpp"
#include "ed_split.hpp"
#include "ed_tables.hpp"
#include "ed_host.hpp"

struct ed_sector;

// Functions that cross a unit boundary and are called from this header
// (global, like ed_err_slot): the process-wide state behind them is defined
// in ed_lib.hip.
// Blocks of `fn` the whole chip holds at once, cached per kernel and LDS size
int resident_grid(const void* fn, int block, size_t lds = 0);
// Pinned host staging from the process-wide pool
void* pinned_get(size_t n);
void pinned_put(void* p);
// ed_hxv.hip: out of line because it takes a kernel's address
int fused_grid(const ed_sector* s, int vc);

namespace edg {

static constexpr int kMaxGrid = 65536;  // one thread per row up to 16.7 M rows
static inline int grid_for(int64_t nthreads) {
  int64_t b = (nthreads + kBlock - 1) / kBlock;
  return (int)std::max<int64_t>(1, std::min<int64_t>(b, kMaxGrid));
}
// one-off grid reductions (in-kernel ticket): few enough blocks that the
// ticket word does not serialise (grid-strided kernels)
static inline int grid_once(int64_t nthreads) { return std::min(grid_for(nthreads), 512); }
// -------------------------------------------------------------- sector obj
struct KronHost {
  int64_t dimup = 0, dimdw = 0;
  int degup = 0, degdw = 0, nimp = 0;
  bool diag_real = true;  // spin-factor diagonals have no imaginary part
  int32_t *upc = nullptr, *dwc = nullptr;
  void *upv = nullptr, *dwv = nullptr, *aup = nullptr, *adw = nullptr;
  double* uimp = nullptr;
  uint8_t *impu = nullptr, *impd = nullptr;
  // two-pass form (k_kron_up + k_kron_dw): up-hop words {col:16 | value index:8}
  bool two = false;
  int cpt = 0, degU = 0, degD = 0;  // template values: columns per thread, slot bounds
  uint32_t *upw = nullptr, *dwo = nullptr;
  uint8_t* dwi = nullptr;
  void *updict = nullptr, *dwdict = nullptr;
  int nupdict = 0, ndwdict = 0;
};

struct LancWS {
  int vc = -1;
  int cap = 0;                  // alpha/beta capacity
  void *R = nullptr, *P = nullptr, *W = nullptr, *Y = nullptr;
  LancState* st = nullptr;
  double* partials = nullptr;   // [kMaxGrid]
  unsigned int* counter = nullptr;
  double *alpha = nullptr, *beta = nullptr, *z = nullptr;  // one block: alpha | beta | z, cap+2 each
  double* h_ab = nullptr;       // pinned host staging for alpha | beta (2*(cap+2)); the persistent kernel of a single run writes it directly
  hipEvent_t ev[2] = {nullptr, nullptr};  // lanc_run timing
  void* basis = nullptr;
  int basis_cols = 0;
};

}  // namespace edg

struct ed_sector {
  int device = 0;
  std::mutex build_mu;  // lazy table builds (ensure_direct)
  hipStream_t stream = nullptr;  // private stream for synchronous entry points
  bool own_stream = true;        // false: the caller's stream (ed_sector_create's argument)
  edg::EdModel Mh;
  edg::EdModel* Md = nullptr;
  edg::SectorTables T;
  int flags = 0;
  int opts = 0;        // ED_OPT_* kernel alternatives (ed_sector_set_options)
  bool hc = true;      // complex H values
  int64_t dim = 0, nslice = 0;
  // rows of the operator held here: [row0, row0+nrows) of the sector (the
  // reference's MPI row split, ED_HAMILTONIAN.f90:55-62); whole sector: 0, dim
  int64_t row0 = 0, nrows = 0;
  int32_t* d_off = nullptr;
  uint32_t* d_rank = nullptr;
  uint32_t* d_map = nullptr;
  // stored (SELL-64)
  void* d_diag = nullptr;
  int64_t* d_sptr = nullptr;
  int32_t* d_cols = nullptr;
  void* d_vals = nullptr;
  uint16_t* d_cnt = nullptr;
  int64_t nnz = 0, padded = 0;
  // packed stored H (real values, <= 256 distinct): {col:24 | index:8} words
  uint32_t* d_words = nullptr;
  void* d_pdict = nullptr;   // real(8) or complex(8) values (hc)
  int npdict = 0;
  // two-segment stored H (ed_split.hpp): A words (diagonal + in-block
  // elements, row order), B slices (cross-block elements: U list + L words)
  bool split = false;
  int64_t* d_sptrA = nullptr;
  uint32_t* d_wordsA = nullptr;
  int64_t paddedA = 0;
  int wA_max = 0, wA_min = 0;  // widest / narrowest A slice (k_spmv_sa chunk choice)
  int64_t split_meta = 0, split_listR = 0;  // (ed_sector_info.split_bytes)
  int split_uch = 8;        // U batch of k_spmv_sb (7 or 8)
  edg::SplitSlice* d_bsl = nullptr;
  int nbsl = 0;
  // k_spmv_sb work lists (half-chunk-major), each cut into 8 per-XCD ranges:
  // real vectors: items of two 64-row halves of pair slices + the generic
  // slices; complex vectors: every half
  int2* d_itR = nullptr;
  int* d_glist = nullptr;
  int* d_xoff = nullptr;    // [27]: items R | generic | items C ranges
  int2* d_ul = nullptr;
  uint32_t* d_lw = nullptr;
  int64_t nul = 0, nlw = 0, nfar = 0, nfar_u = 0;  // U entries, L words, cross-block elements (all / in U)
  // fused one-pass re-laid stored H (ed_fused.hpp): 64-row units of one idw
  // block with A words (in-block), U list (unit-uniform cross-block), L words
  bool fused = false;
  edg::FuUnit* d_fu = nullptr;
  int64_t nfu = 0;
  uint32_t* d_fa = nullptr;
  int2* d_ful = nullptr;
  uint32_t* d_flw = nullptr;
  int64_t fu_na = 0, fu_nu = 0, fu_nl = 0, fu_far = 0, fu_far_u = 0;  // A words, U entries, L words, cross (all / U)
  int fu_wa_max = 0, fu_wa_min = 0, fu_uch = edg::kFuUChunk;
  // matrix-free, generic (k_direct): chunk list, per-block op lists, 16-bit tables
  edg::DirChunk* d_dchunk = nullptr;   // 64-row chunks (real vectors)
  int ndchunk = 0;
  edg::DirChunk* d_dchunk2 = nullptr;  // 128-row chunks (complex vectors, two rows per lane)
  int ndchunk2 = 0;
  edg::DirGroup* d_dops = nullptr;
  uint16_t *d_rank16 = nullptr, *d_pat16 = nullptr;
  void* d_ddiag = nullptr;   // gen_diag of the sector object's rows (k_gen_diag)
  bool dir_patlds = false;
  int dir_lds = 0, dir_grid = 0;
  // matrix-free, Kronecker form
  bool kron = false;
  edg::KronHost K;
  // host-pointer H·v staging
  void *d_x = nullptr, *d_y = nullptr;
  edg::LancWS ws;
  int64_t bytes = 0;
  std::vector<void*> allocs;
  // persistent one-workgroup Lanczos (small sectors)
  double pthresh = 0.0;     // breakdown threshold of the current persistent run
  // the last persist_mode answer and its LDS bytes, valid for (vc, path, opts);
  // one entry: the mode's tables (MODE 4: per path) are those of the last answer
  struct {
    int vc = -1, path = -3, opts = 0, mode = -1;
    int64_t lds = 0;
  } pchoice;
  // register-resident stored matrix for the persistent kernel (MODE 2)
  int preg_E = 0;           // 0 not built, -1 ineligible, else ELL row width W
  int preg_rpt = 0;         // rows per thread (template value)
  int kreg_W = 0, kreg_rpt = 0;  // MODE 3 (Kronecker words in registers)
  uint32_t* d_pk = nullptr;
  void* d_dict = nullptr;
  int ndict = 0;
  // Kronecker register layout for the persistent kernel (MODE 4)
  int pkr_state = 0;        // 0 not tried, -1 ineligible, 1 tables ready
  int pkr_src = -1;         // path the tables came from (0 stored SELL, 2 hop tables)
  int pkr_E = 0, pkr_rpt = 0, pkr_du = 0, pkr_dd = 0, pkr_degu = 0, pkr_degd = 0;
  const int32_t *d_kupc = nullptr, *d_kdwc = nullptr;
  const double *d_kupv = nullptr, *d_kdwv = nullptr, *d_kdiag = nullptr;
  // graph cache for Lanczos iterations
  hipGraphExec_t gexec = nullptr;
  int g_path = -2, g_vc = -1, g_chunk = 0;
  bool g_basis = false;
};

namespace edg {

// All device memory and copies of a sector are ordered on its private stream
// (stream-ordered allocator, async copies + a stream sync): no call here
// synchronises the device or the null stream, so sectors can be built,
// solved (graph capture included) and freed from several host threads at
// once (farm workers).
static int dcopy(const ed_sector* s, void* dst, const void* src, size_t n, hipMemcpyKind k) {
  HIPCK(hipMemcpyAsync(dst, src, n, k, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  return ED_OK;
}
static int dalloc(ed_sector* s, void** p, size_t n) {
  if (n == 0) n = 16;
  hipError_t e = hipMallocAsync(p, n, s->stream);
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? ED_ERR_OOM : ED_ERR_HIP,
                std::string("hipMalloc(") + std::to_string(n) + ") -> " + hipGetErrorString(e));
  }
  s->allocs.push_back(*p);
  s->bytes += (int64_t)n;
  return ED_OK;
}
static void dfree(ed_sector* s, void** p, size_t n) {
  if (!*p) return;
  auto it = std::find(s->allocs.begin(), s->allocs.end(), *p);
  if (it != s->allocs.end()) s->allocs.erase(it);
  (void)hipFreeAsync(*p, s->stream);
  s->bytes -= (int64_t)n;
  *p = nullptr;
}
template <class T>
static int dalloc_t(ed_sector* s, T** p, size_t count) {
  return dalloc(s, (void**)p, count * sizeof(T));
}
template <class T>
static int upload(ed_sector* s, T** p, const std::vector<T>& h) {
  CK(dalloc_t(s, p, h.size()));
  return dcopy(s, *p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// A pool block for one solve on stream st, returned only once st is idle (it
// is on the success path; after an early error return a copy may still be in
// flight, and the block must not reach another thread under it).
struct PinnedLease {
  void* const p;
  const hipStream_t st;
  PinnedLease(size_t n, hipStream_t st_) : p(pinned_get(n)), st(st_) {}
  PinnedLease(const PinnedLease&) = delete;
  ~PinnedLease() {
    if (!p) return;
    (void)hipStreamSynchronize(st);
    pinned_put(p);
  }
};
struct DevFree {  // hipFreeAsync of one device block at scope exit
  void* p;
  hipStream_t st;
  ~DevFree() {
    if (p) (void)hipFreeAsync(p, st);
  }
};
// f(std::true_type) for complex(8) vectors, f(std::false_type) for real ones:
// one generic lambda over the vector type where a call or a launch would
// otherwise stand twice
template <class F>
static inline auto with_vc(bool vc, F&& f) {
  return vc ? f(std::true_type{}) : f(std::false_type{});
}
// sub-arrays of a device slice of doubles start on 16-byte boundaries (double2)
static inline size_t even(size_t q) { return (q + 1) & ~(size_t)1; }

// Row-split sectors (ed_sector_create_rows) hold rows [row0, row0+nrows) of
// H: H·v from a whole-sector vector and the CSR dump only.
static int whole_only(const ed_sector* s) {
  if (s->nrows == s->dim) return ED_OK;
  return fail(ED_ERR_UNSUPPORTED, "row-split sector: only ed_sector_hxv_dev[_path] and ed_sector_dump_csr apply");
}

// Bytes of the stored matrix stream (the NT threshold: beyond ~192 MB it
// cannot stay in the 256 MB MALL next to the vectors).
static int64_t stored_mbytes(const ed_sector* s) {
  const int64_t hv = s->hc ? 16 : 8;
  if (s->d_words) return s->padded * 4 + s->nrows * hv;
  return s->padded * (4 + hv) + s->nrows * hv;
}
// the two-segment form (ed_build.hip: build_split) is built, and its launch
// shapes chosen, from this size on
static constexpr int64_t kSplitMinBytes = (int64_t)192 << 20;

template <bool HC>
static KronArgs<HC> kron_args(const ed_sector* s) {
  using H = val_t<HC>;
  KronArgs<HC> a;
  a.dimup = s->K.dimup; a.dimdw = s->K.dimdw; a.degup = s->K.degup; a.degdw = s->K.degdw;
  a.nimp = s->K.nimp;
  a.upc = s->K.upc; a.upv = (const H*)s->K.upv; a.dwc = s->K.dwc; a.dwv = (const H*)s->K.dwv;
  a.aup = (const H*)s->K.aup; a.adw = (const H*)s->K.adw; a.uimp = s->K.uimp;
  a.impu = s->K.impu; a.impd = s->K.impd;
  return a;
}

// ------------------------------------------------------------ H·v launch
// path: 0 = stored SELL, 1 = direct generic, 2 = direct Kronecker, -1 = default
static int resolve_path(const ed_sector* s, int path) {
  if (path == -1) {
    if (s->flags & ED_STORED) return 0;
    return s->kron ? 2 : 1;
  }
  if (path == 0 && !(s->flags & ED_STORED)) return -1;
  if (path == 2 && !s->kron) return -1;
  if (path < 0 || path > 2) return -1;
  return path;
}

// XCD-aware block order for the stored kernels (each XCD sweeps one row
// range, so its L2 serves the v gathers of neighbouring rows): n28 packed
// 0.240 -> 0.230 ms, c4 0.0193 -> 0.0173 ms.  The grid is then a multiple of
// 8; every per-block reduction over an H·v launch must use hxv_blocks().
// Only the packed kernel on grids of >= 1024 blocks gains (plain SELL n28:
// 0.421 -> 0.443 ms with the remap; small grids lose blocks to the rounding).
static bool xcd_on(const ed_sector* s, int path) {
  return path == 0 && s->d_words && grid_for(s->nslice * 64) >= 1024;
}
// pass D of the two-pass Kronecker H·v: a multiple of 8 blocks (XCD column
// chunks), 8 resident per CU
static constexpr int kKronDwGrid = 2048;
static constexpr int kKronDwGrid2 = 1280;  // two columns per lane
// pass U LDS: dictionary + two sets of `rows` staged rows
static constexpr int kKronUpSets = 2;
static size_t kron_up_lds(bool hc, bool vc, int64_t du, int rows) {
  return kKronDictMax * (hc ? 16 : 8) + kKronUimpMax * 8 + kKronUpSets * rows * (size_t)((du + 1) & ~1) * (vc ? 16 : 8);
}
static int kron_up_rows(bool hc, bool vc, int64_t du) { return kron_up_lds(hc, vc, du, 2) <= 160 * 1024 ? 2 : 1; }
static bool kron2_on(const ed_sector* s, int path, int vc) {
  if (path != 2 || !s->K.two) return false;
  return kron_up_lds(s->hc, vc, s->K.dimup, 1) <= 160 * 1024;
}
// pass D grid: kKronDwGrid blocks (a multiple of 8: XCD column chunks).
// Every per-block reduction of a pass-D epilogue is sized by this (through
// hxv_blocks).
// Complex vectors take half the grid: their column chunk V[:, c0:c0+64] is
// twice the bytes, and fewer chunks in flight keep it in L2 (N28 complex
// pass D: 512 blocks 187-193 us, 1024 160 us, 2048 167 us; real: 109, 81, 80).
// The two-column real form (even DimUp) has twice the chunk bytes too and
// takes 1280 blocks, 5 per CU (N28: 2048 0.111 ms, 1536 0.115, 1280 0.104-
// 0.106, 1024 0.104, 768 0.106-0.107; N28b 0.134 / 0.129 / 0.126-0.131 /
// 0.129-0.130 / 0.135; configs[3] (6,6) 0.0150 / 0.0152 / 0.0152-0.0153 /
// 0.0155 / 0.0161 ms).
static int kron_dw_grid(const ed_sector* s, bool vc) {
  if (vc) return kKronDwGrid / 2;
  // (a launch whose pointers are not 16-byte aligned falls back to the
  // one-column form on this same grid: hxv_blocks() must match the launch)
  return s->K.dimup % 2 == 0 ? kKronDwGrid2 : kKronDwGrid;
}
// the two-segment stored kernels serve path 0 unless ED_OPT_STORED_EXACT
// The fused form serves complex(8) vectors, and real vectors where the
// two-segment form is not built (its y round trip stays in the Infinity Cache
// for real vectors: N28 0.182 ms against 0.186 fused, gpurun_out r6b).
static bool fused_on(const ed_sector* s, int path, int vc) {
  return path == 0 && s->fused && !(s->opts & (ED_OPT_STORED_EXACT | ED_OPT_NO_FUSED)) && (vc || !s->split);
}
static bool split_on(const ed_sector* s, int path, int vc = 0) {
  // (real vectors only: with complex(8) vectors x and y do not fit the
  // Infinity Cache together and the split is slower than one pass, N28 0.359
  // against 0.316 ms)
  return path == 0 && s->split && !vc && !(s->opts & ED_OPT_STORED_EXACT);
}
static int hxv_blocks(const ed_sector* s, int path, int vc = 0) {
  if (kron2_on(s, path, vc)) return kron_dw_grid(s, vc);
  if (fused_on(s, path, vc)) return fused_grid(s, vc);
  if (split_on(s, path, vc)) return kSplitGrid;
  if (path == 1) return s->dir_grid;
  const int g = grid_for(s->nslice * 64);
  return xcd_on(s, path) ? (g & ~7) : g;
}

}  // namespace edg

// ---------------------------------- the other functions that cross the units
// ed_hxv.hip: launch_hxv is instantiated there for VC in {false, true} x
// {EpiStore, EpiTrlLoc, EpiLancA}, so every H·v kernel is compiled once
template <bool VC, class Epi>
int launch_hxv(ed_sector* s, int path, const void* x, Epi epi, hipStream_t st);
// ed_multi.hip: the block stored kernel k_spmv_mv (ed_multi.hpp) on x, a
// dim x NV row-interleaved block; instantiated there for VC in {false, true}
// x NV in {1, 2, 4, 8} x {EpiStoreMV, EpiLancAMV}.  hxv_mv_blocks: its grid;
// mv_sector_check: ED_ERR_UNSUPPORTED unless the sector is stored and whole
template <bool VC, int NV, class Epi>
int launch_hxv_mv(ed_sector* s, const void* x, Epi epi, hipStream_t st);
int hxv_mv_blocks(const ed_sector* s);
int mv_sector_check(const ed_sector* s);
// ed_build.hip: the builders sector_create (ed_lib.hip) runs, each on the
// sector's stream, and the k_direct tables on first use of path 1
int build_map(ed_sector* s);
int build_stored(ed_sector* s);
int build_kron(ed_sector* s);
int build_direct(ed_sector* s);
int ensure_direct(ed_sector* s, int path, hipStream_t caller = nullptr);
// ed_lanczos.hip: the captured recurrence of a sector is dropped when its
// options change (ed_sector_set_options, ed_lib.hip)
void drop_graph(ed_sector* s);
// ed_lanczos.hip: k_default_start on n doubles (the eigensolver's default
// start vector is the Lanczos one; the kernel is compiled once, there)
void launch_default_start(double* v, int64_t n, hipStream_t st);
