// ed_lib.hip — the sector object's life cycle and the library's process-wide
// state (the error slot, the resident_grid cache, the pinned pool), the
// sector entry points of the C-ABI (include/ed_gpu.h) and the reference-style
// singleton API with its globals.  The sector object itself is in
// ed_sector.hpp; the units over it: the H builders in ed_build.hip, the H·v
// launchers in ed_hxv.hip, the plain and persistent Lanczos drivers in
// ed_lanczos.hip, the thick-restart eigensolver in ed_eigh.hip.
#include "ed_sector.hpp"

using namespace edg;

// ------------------------------------------------------------------ errors
// (fail / HIPCK / CK in ed_host.hpp; the message slot is this TU's)
std::string& ed_err_slot() {
  static thread_local std::string e;
  return e;
}

// Blocks of `fn` the whole chip holds at once (occupancy x CUs, a multiple of
// the 8 XCDs): the grid of a grid-strided kernel whose blocks have equal
// work, so that no block waits for a second round (a 2,048-block grid at 5
// resident blocks per CU runs 1,280 + 768).
int resident_grid(const void* fn, int block, size_t lds) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({fn, lds});
  if (it != cache.end()) return it->second;
  int per = 0, dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, block, lds) != hipSuccess)
    return 1024;
  const int g = std::max(8, (std::max(per, 1) * ncu) & ~7);
  cache[{fn, lds}] = g;
  return g;
}

// Pinned host staging, every buffer of the library (a sector's plain-Lanczos
// alpha|beta copies; the thick-restart, batch and lockstep solves' per-call
// staging through PinnedLease), from a process-wide pool that only grows:
// hipHostFree / hipHostMalloc synchronise the device, which would stall every
// other worker thread's stream (and break their graph captures), so nothing
// is freed while the library is in use.  Blocks belong to no host thread:
// short-lived threads (a farm call's workers) leak none.
static std::mutex g_pin_mu;
static std::multimap<size_t, void*> g_pin_free;  // free blocks by size
static std::map<void*, size_t> g_pin_size;       // every block ever allocated
void* pinned_get(size_t n) {
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pin_free.lower_bound(n);
    if (it != g_pin_free.end()) {
      void* p = it->second;
      g_pin_free.erase(it);
      return p;
    }
  }
  n = std::max<size_t>(n, 4096);
  void* p = nullptr;
  if (hipHostMalloc(&p, n, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_size[p] = n;
  return p;
}
void pinned_put(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_free.emplace(g_pin_size[p], p);
}

static void sector_free(ed_sector* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
  for (hipEvent_t& e : s->ws.ev)
    if (e) (void)hipEventDestroy(e);
  if (s->stream) {
    for (void* p : s->allocs) (void)hipFreeAsync(p, s->stream);
    (void)hipStreamSynchronize(s->stream);
    if (s->own_stream) (void)hipStreamDestroy(s->stream);
  }
  pinned_put(s->ws.h_ab);  // after the stream sync above: no copy into it is in flight
  delete s;
}

// ---------------------------------------------------------------- C-ABI
extern "C" {

const char* ed_gpu_last_error(void) { return ed_err_slot().c_str(); }

// Jz_basis sectors: every off-diagonal element must land inside the sector
// (the reference would insert it at column binary_search(...) = 0).  Host
// pass over the sector with the element generator, before any device build.
struct JzCheckAcc {
  const SectorTables* T;
  bool ok = true;
  void diag(double, double) {}
  void off(uint32_t k, double, double) { ok = ok && table_index(*T, k) >= 0; }
};
static bool jz_conserved(const EdModel& M, const SectorTables& T) {
  JzCheckAcc acc;
  acc.T = &T;
  for (size_t b = 0; b + 1 < T.blk_off.size() && acc.ok; b++) {
    const uint32_t idw = T.blk_idw[b];
    const int32_t c0 = T.cls_start[T.need_cls[idw]];
    for (int64_t r = 0; r < T.blk_off[b + 1] - T.blk_off[b] && acc.ok; r++)
      gen_row(M, T.by_cls[c0 + r] | (idw << T.ns), acc);
  }
  return acc.ok;
}

static int sector_create(const ed_params* p, int32_t q1, int32_t q2, int32_t flags, int64_t row0,
                         int64_t nrows, int32_t device, hipStream_t stream, ed_sector** out) {
  if (!out) return fail(ED_ERR_ARG, "out == NULL");
  *out = nullptr;
  if (!(flags & (ED_STORED | ED_DIRECT))) return fail(ED_ERR_ARG, "flags need ED_STORED or ED_DIRECT");
  int ndev = 0;
  HIPCK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(ED_ERR_ARG, "bad device ordinal");
  HIPCK(hipSetDevice(device));
  ed_sector* s = new ed_sector();
  s->device = device;
  int rc = model_from_params(p, &s->Mh);
  if (rc != ED_OK) {
    delete s;
    return fail(rc, "invalid ed_params (Norb/Nspin/Nbath/ed_mode/bath_type)");
  }
  const bool real_ok = model_is_real(s->Mh);
  if ((flags & ED_REAL) && !real_ok) {
    delete s;
    return fail(ED_ERR_ARG, "ED_REAL requested but impHloc/bath carry imaginary parts");
  }
  s->hc = !(flags & ED_REAL);
  s->flags = flags;
  rc = build_tables(s->Mh.ns, s->Mh.mode, q1, (s->Mh.mode == ED_MODE_NORMAL || s->Mh.jz) ? q2 : 0, &s->T,
                    s->Mh.jz ? s->Mh.lz2 : nullptr);
  if (rc != ED_OK) {
    delete s;
    return fail(rc, "sector tables: bad quantum numbers or dimension beyond int32");
  }
  if (s->T.dim == 0) {
    delete s;
    return fail(ED_ERR_ARG, "empty sector");
  }
  if (s->Mh.jz && !jz_conserved(s->Mh, s->T)) {
    delete s;
    return fail(ED_ERR_UNSUPPORTED,
                "Jz_basis: H moves states out of the (n, twoJz) sector (impHloc / bath / Jp not Jz-conserving)");
  }
  s->dim = s->T.dim;
  if (nrows < 0) {
    row0 = 0;
    nrows = s->dim;
  }
  if (row0 < 0 || nrows < 0 || row0 + nrows > s->dim) {  // nrows == 0: a rank with no rows (dim < MpiSize)
    delete s;
    return fail(ED_ERR_ARG, "row range outside the sector");
  }
  s->row0 = row0;
  s->nrows = nrows;
  s->nslice = (nrows + 63) / 64;
#define TRY(x)            \
  do {                    \
    int r2_ = (x);        \
    if (r2_ != ED_OK) {   \
      sector_free(s);     \
      return r2_;         \
    }                     \
  } while (0)
  // a caller's stream (a farm worker's, reused for every sector it solves)
  // or a private non-blocking one
  hipError_t he = hipSuccess;
  if (stream) {
    s->stream = stream;
    s->own_stream = false;
  } else {
    he = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  }
  if (he != hipSuccess) {
    delete s;
    return fail(ED_ERR_HIP, "hipStreamCreate");
  }
  TRY(dalloc_t(s, &s->Md, 1));
  if (dcopy(s, s->Md, &s->Mh, sizeof(EdModel), hipMemcpyHostToDevice) != ED_OK) {
    sector_free(s);
    return fail(ED_ERR_HIP, "model upload");
  }
  TRY(upload(s, &s->d_off, s->T.off));
  TRY(upload(s, &s->d_rank, s->T.rank));
  TRY(build_map(s));
  // Kronecker form: normal mode without Jx/Jp terms (no term moves both spins)
  s->kron = (flags & ED_DIRECT) && s->Mh.mode == ED_MODE_NORMAL && !s->Mh.jhflag && nrows == s->dim;
  if ((flags & ED_STORED) && nrows > 0) TRY(build_stored(s));
  if (s->kron) TRY(build_kron(s));
  // k_direct tables: built here only when the generic matrix-free kernel is
  // the sector's default H·v; otherwise on the first explicit path-1 request
  // (ensure_direct), so stored, Kronecker and GF source sectors keep their
  // build cost and failure modes
  if ((flags & ED_DIRECT) && nrows > 0 && resolve_path(s, -1) == 1) TRY(build_direct(s));
  if (hipStreamSynchronize(s->stream) != hipSuccess) {
    sector_free(s);
    return fail(ED_ERR_HIP, "sector build");
  }
#undef TRY
  *out = s;
  return ED_OK;
}

int ed_sector_create(const ed_params* p, int32_t q1, int32_t q2, int32_t flags, int32_t device,
                     void* stream, ed_sector** out) {
  return sector_create(p, q1, q2, flags, 0, -1, device, (hipStream_t)stream, out);
}

int ed_sector_create_rows(const ed_params* p, int32_t q1, int32_t q2, int32_t flags, int64_t row0,
                          int64_t nrows, int32_t device, void* stream, ed_sector** out) {
  return sector_create(p, q1, q2, flags, row0, nrows, device, (hipStream_t)stream, out);
}

int ed_sector_destroy(ed_sector* s) {
  sector_free(s);
  return ED_OK;
}

// every defined ED_OPT_* bit (include/ed_gpu.h); any other bit is refused
static constexpr int32_t kOptKnown =
    ED_OPT_NO_PERSIST | ED_OPT_PERSIST_STORED | ED_OPT_NO_PREG | ED_OPT_NO_PKRON | ED_OPT_SPLIT_SIMPLE |
    ED_OPT_NO_BATCH | ED_OPT_EIGH_NO_VERIFY | ED_OPT_TRLAN_UNFUSED | ED_OPT_TRLAN_NOFOLD | ED_OPT_NO_GRAPH |
    ED_OPT_TRLAN_NOLOCAL | ED_OPT_TRLAN_NOSOLO | ED_OPT_TRLAN_FULLUPD | ED_OPT_STORED_EXACT |
    ED_OPT_EIGH_FULLPROBE | ED_OPT_NO_FUSED | ED_OPT_EIGH_NOHINT | ED_OPT_TWIN_GATHER;

int ed_sector_set_options(ed_sector* s, int32_t opts) {
  if (!s) return fail(ED_ERR_ARG, "null");
  if (opts & ~kOptKnown) return fail(ED_ERR_ARG, "unknown ED_OPT_* bits");
  if (opts != s->opts) {
    drop_graph(s);  // a captured recurrence bakes in the kernel choice
    s->pchoice.vc = -1;  // and the persistent mode is chosen anew
  }
  s->opts = opts;
  return ED_OK;
}

int ed_sector_get_info(const ed_sector* s, ed_sector_info* info) {
  if (!s || !info) return fail(ED_ERR_ARG, "null");
  memset(info, 0, sizeof(*info));
  info->dim = s->dim;
  info->row0 = s->row0;
  info->nrows = s->nrows;
  info->nnz = (s->flags & ED_STORED) ? s->nnz : 0;
  info->padded = s->padded;
  info->ns = s->Mh.ns;
  info->mode = s->Mh.mode;
  info->q1 = s->T.q1;
  info->q2 = s->T.q2;
  info->flags = s->flags;
  info->kron = s->kron ? 1 : 0;
  info->dimup = s->T.dimup;
  info->dimdw = s->T.dimdw;
  info->device_bytes = s->bytes;
  info->packed = s->d_words ? 1 : 0;
  info->npdict = s->npdict;
  info->split = s->split ? 1 : 0;
  info->split_far = s->nfar;
  info->split_far_uniform = s->nfar_u;
  info->fused = s->fused ? 1 : 0;
  info->fused_far = s->fu_far;
  info->fused_far_uniform = s->fu_far_u;
  info->fused_bytes = s->fused ? (s->fu_na + s->fu_nl) * 4 + s->fu_nu * 8 + s->nfu * (int64_t)sizeof(FuUnit) : 0;
  info->split_bytes = s->split ? (s->paddedA + s->nlw) * 4 + s->nul * 8 + s->split_meta : 0;
  info->split_list_bytes = s->split ? s->split_listR : 0;
  return ED_OK;
}

int ed_sector_map(const ed_sector* s, uint32_t* map_host) {
  if (!s || !map_host) return fail(ED_ERR_ARG, "null");
  HIPCK(hipSetDevice(s->device));
  CK(dcopy(s, map_host, s->d_map, s->dim * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return ED_OK;
}

int ed_sector_dump_csr(const ed_sector* s, int64_t* rowptr, int32_t* cols, double* vals) {
  if (!s || !rowptr || !cols || !vals) return fail(ED_ERR_ARG, "null");
  if (!(s->flags & ED_STORED)) return fail(ED_ERR_STATE, "sector was built without ED_STORED");
  HIPCK(hipSetDevice(s->device));
  const int64_t dim = s->nrows, ns = s->nslice, slots = s->padded;  // local rows, global columns
  rowptr[0] = 0;
  if (dim == 0) return ED_OK;
  const int hw = s->hc ? 2 : 1;
  std::vector<uint16_t> cnt(dim);
  std::vector<int64_t> sptr(ns + 1);
  std::vector<int32_t> sc(slots);
  std::vector<double> sv(slots * hw), dg(dim * hw);
  CK(dcopy(s, cnt.data(), s->d_cnt, dim * 2, hipMemcpyDeviceToHost));
  CK(dcopy(s, sptr.data(), s->d_sptr, (ns + 1) * 8, hipMemcpyDeviceToHost));
  CK(dcopy(s, sc.data(), s->d_cols, slots * 4, hipMemcpyDeviceToHost));
  CK(dcopy(s, sv.data(), s->d_vals, slots * 8 * hw, hipMemcpyDeviceToHost));
  CK(dcopy(s, dg.data(), s->d_diag, dim * 8 * hw, hipMemcpyDeviceToHost));
  int64_t q = 0;
  rowptr[0] = 0;
  for (int64_t i = 0; i < dim; i++) {
    cols[q] = (int32_t)(s->row0 + i);
    vals[2 * q] = dg[hw * i];
    vals[2 * q + 1] = hw == 2 ? dg[2 * i + 1] : 0.0;
    q++;
    int64_t base = sptr[i >> 6] + (i & 63);
    for (int k = 0; k < cnt[i]; k++) {
      int64_t t = base + 64 * (int64_t)k;
      cols[q] = sc[t];
      vals[2 * q] = sv[hw * t];
      vals[2 * q + 1] = hw == 2 ? sv[2 * t + 1] : 0.0;
      q++;
    }
    rowptr[i + 1] = q;
  }
  return ED_OK;
}

int ed_sector_sell_view(const ed_sector* s, ed_sell_view* v) {
  if (!s || !v) return fail(ED_ERR_ARG, "null");
  if (!(s->flags & ED_STORED)) return fail(ED_ERR_STATE, "sector was built without ED_STORED");
  v->dim = s->dim;
  v->nslice = s->nslice;
  v->slots = s->padded;
  v->value_bytes = s->hc ? 16 : 8;
  v->pad = 0;
  v->diag = s->d_diag;
  v->sptr = s->d_sptr;
  v->cols = s->d_cols;
  v->vals = s->d_vals;
  v->rowcnt = s->d_cnt;
  return ED_OK;
}

// ------------------------------------------------- reference-style globals
static std::mutex g_mu;
static ed_params g_params;
static bool g_have_params = false;
static int g_device = 0;
static ed_sector* g_cur = nullptr;

int ed_gpu_init(const ed_params* p) {
  if (!p) return fail(ED_ERR_ARG, "null params");
  EdModel M;
  int rc = model_from_params(p, &M);
  if (rc != ED_OK) return fail(rc, "invalid ed_params");
  std::lock_guard<std::mutex> lk(g_mu);
  g_params = *p;
  g_have_params = true;
  return ED_OK;
}

int ed_gpu_set_device(int32_t device) {
  int n = 0;
  HIPCK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(ED_ERR_ARG, "bad device");
  g_device = device;
  return ED_OK;
}

int ed_gpu_build_sector(int32_t q1, int32_t q2, int32_t flags, int64_t* dim) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_have_params) return fail(ED_ERR_STATE, "ed_gpu_init not called");
  if (g_cur) {  // build_Hv_sector on a live sector: replace it
    sector_free(g_cur);
    g_cur = nullptr;
  }
  CK(ed_sector_create(&g_params, q1, q2, flags, g_device, nullptr, &g_cur));
  if (dim) *dim = g_cur->dim;
  return ED_OK;
}

int ed_gpu_vecdim(int32_t* vecdim) {
  if (!g_cur || !vecdim) return fail(ED_ERR_STATE, "no current sector");
  *vecdim = (int32_t)g_cur->nrows;  // MpiQ + MpiR (ED_HAMILTONIAN.f90:126-149); serial: Dim
  return ED_OK;
}

int ed_gpu_mpi_split(int64_t dim, int32_t rank, int32_t size, int64_t* row0, int64_t* nrows) {
  if (!row0 || !nrows || size < 1 || rank < 0 || rank >= size || dim < 0) return fail(ED_ERR_ARG, "mpi_split args");
  const int64_t q = dim / size;                          // MpiQ
  const int64_t r = rank == size - 1 ? dim % size : 0;   // MpiR (last rank)
  *row0 = (int64_t)rank * q;                             // MpiIshift
  *nrows = q + r;                                        // MpiIend - MpiIstart + 1
  return ED_OK;
}
int ed_gpu_build_sector_rows(int32_t q1, int32_t q2, int32_t flags, int64_t row0, int64_t nrows, int64_t* dim) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_have_params) return fail(ED_ERR_STATE, "ed_gpu_init not called");
  if (g_cur) {
    sector_free(g_cur);
    g_cur = nullptr;
  }
  CK(ed_sector_create_rows(&g_params, q1, q2, flags, row0, nrows, g_device, nullptr, &g_cur));
  if (dim) *dim = g_cur->dim;
  return ED_OK;
}
int ed_gpu_hxv_mpi(const int32_t* nloc, const double* vin, double* hv) {
  if (!g_cur) return fail(ED_ERR_STATE, "ed_gpu_hxv_mpi ERROR: Hsector NOT set");
  if (!nloc) return fail(ED_ERR_ARG, "null");
  ed_sector* s = g_cur;
  if ((int64_t)*nloc != s->nrows) return fail(ED_ERR_ARG, "ed_gpu_hxv_mpi ERROR: Nloc != local rows of the sector");
  if (s->nrows == 0) return ED_OK;
  if (!vin || !hv) return fail(ED_ERR_ARG, "null");
  HIPCK(hipSetDevice(s->device));
  if (!s->d_x) {
    CK(dalloc(s, &s->d_x, s->dim * 16));
    CK(dalloc(s, &s->d_y, s->nrows * 16));
  }
  HIPCK(hipMemcpyAsync(s->d_x, vin, s->dim * 16, hipMemcpyHostToDevice, s->stream));
  CK(ed_sector_hxv_dev(s, 1, s->d_x, s->d_y, s->stream));
  HIPCK(hipMemcpyAsync(hv, s->d_y, s->nrows * 16, hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  return ED_OK;
}
int ed_gpu_hxv(const int32_t* nloc, const double* v, double* hv) {
  if (!g_cur) return fail(ED_ERR_STATE, "ed_gpu_hxv ERROR: Hsector NOT set");
  if (!nloc) return fail(ED_ERR_ARG, "null nloc");
  return ed_sector_hxv(g_cur, *nloc, v, hv);
}

int ed_gpu_nnz(int64_t* nnz) {
  if (!g_cur) return fail(ED_ERR_STATE, "no current sector");
  if (!nnz) return fail(ED_ERR_ARG, "null");
  if (!(g_cur->flags & ED_STORED)) return fail(ED_ERR_STATE, "sector was built without ED_STORED");
  *nnz = g_cur->nnz;
  return ED_OK;
}

int ed_gpu_dump_csr(int64_t* rowptr, int32_t* cols, double* vals) {
  if (!g_cur) return fail(ED_ERR_STATE, "no current sector");
  return ed_sector_dump_csr(g_cur, rowptr, cols, vals);
}

int ed_gpu_lanc_eigh(int32_t nitermax, double threshold, int32_t ncheck, double* egs, double* vect,
                     int32_t* nlanc) {
  if (!g_cur) return fail(ED_ERR_STATE, "no current sector");
  return ed_sector_lanc_eigh(g_cur, 1, nullptr, nitermax, threshold, ncheck, egs, vect, nlanc);
}

int ed_gpu_eigh(int32_t neigen, int32_t nblock, int32_t nitermax, double tol, const double* v0,
                double* evals, double* evecs, int32_t* nconv) {
  if (!g_cur) return fail(ED_ERR_STATE, "no current sector");
  const int64_t dim = g_cur->dim;
  const int ncv = (int)std::min<int64_t>(std::min(std::max(nblock, neigen + 1), 64), dim);
  return ed_sector_eigh(g_cur, 1, neigen, ncv, nitermax, tol, v0, evals, evecs, nconv, nullptr);
}

int ed_gpu_lanc_tridiag(const double* v0, int32_t nitermax, double threshold, double* alfa,
                        double* beta, int32_t* nlanc) {
  if (!g_cur) return fail(ED_ERR_STATE, "no current sector");
  return ed_sector_lanc_tridiag(g_cur, 1, v0, nitermax, threshold, alfa, beta, nlanc);
}

int ed_gpu_delete_sector(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  // delete_Hv_sector: safe after a direct build (the reference stops in
  // sp_delete_matrix there, ED_HAMILTONIAN.f90:111-119 / ED_SPARSE_MATRIX.f90:180)
  if (g_cur) sector_free(g_cur);
  g_cur = nullptr;
  return ED_OK;
}

int ed_gpu_finalize(void) {
  ed_gpu_delete_sector();
  std::lock_guard<std::mutex> lk(g_mu);
  g_have_params = false;
  return ED_OK;
}

int ed_gpu_current_sector(ed_sector** out) {
  if (!out) return fail(ED_ERR_ARG, "null");
  *out = g_cur;
  return g_cur ? ED_OK : fail(ED_ERR_STATE, "no current sector");
}

}  // extern "C"
