// ed_hxv.hip — every H·v launcher (stored, packed, two-segment, fused,
// generic matrix-free, Kronecker one- and two-pass) behind launch_hxv, which
// is instantiated here once per epilogue, and the entry points that apply an
// operator to a vector: H·v, the Kronecker row / column split, c / c^+,
// twin-sector vectors and the observables of a kept state.
#include "ed_sector.hpp"
#include "ed_obs.hpp"
#include "ed_twin.hpp"
#include "ed_seed.hpp"
#include "ed_chi.hpp"

using namespace edg;

namespace edg {
// -------------------------------- row split: columns the held rows gather
// One bit per sector column, set for every column an off-diagonal element of
// rows [row0, row0 + n) refers to (gen_row's elements: stored and matrix-free
// alike).  The halo of a rank's row block for the split H·v (edgpu.dist).
struct MarkAcc {
  DevIndex idx;
  uint32_t* mask;
  __device__ __forceinline__ void diag(double, double) {}
  __device__ __forceinline__ void off(uint32_t k, double, double) {
    const uint32_t c = (uint32_t)idx(k);
    atomicOr(mask + (c >> 5), 1u << (c & 31));
  }
};
static __global__ void __launch_bounds__(kBlock) k_mark_cols(const EdModel* __restrict__ Mp,
                                                      const uint32_t* __restrict__ map, int64_t n,
                                                      DevIndex idx, uint32_t* mask) {
  const EdModel& M = *Mp;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    MarkAcc a{idx, mask};
    gen_row(M, map[i], a);
  }
}
}  // namespace edg

template <bool HC, bool VC, bool PL, class Epi>
static int launch_direct(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  using V = val_t<VC>;
  // the gathers address x through a 4 GiB buffer resource with 32-bit byte
  // offsets (ld_rsrc): a longer vector would read zeros past the range
  if ((uint64_t)s->dim * sizeof(V) > kDirMaxVecBytes)
    return fail(ED_ERR_UNSUPPORTED, "k_direct: vector of " + std::to_string(s->dim) +
                                        " elements exceeds the 4 GiB gather range (use the stored or Kronecker path)");
  constexpr int R = VC ? kDirRows : 1;
  auto fn = k_direct<HC, VC, PL, R, Epi>;
  // dynamic LDS beyond 64 KB: allow what the 160 KB leave next to the
  // function's static LDS (the epilogue's reduction slots)
  static std::once_flag attr;
  static hipError_t ae = hipSuccess;
  std::call_once(attr, [&]() {
    hipFuncAttributes fa{};
    ae = hipFuncGetAttributes(&fa, (const void*)fn);
    if (ae == hipSuccess)
      ae = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024 - (int)fa.sharedSizeBytes);
  });
  if (ae != hipSuccess) {
    (void)hipGetLastError();  // not sticky for later launches
    return fail(ED_ERR_HIP, std::string("k_direct LDS attribute -> ") + hipGetErrorString(ae));
  }
  hipLaunchKernelGGL(fn, dim3(s->dir_grid), dim3(kDirBlock), s->dir_lds, st, (const val_t<HC>*)s->d_ddiag,
                     R == 1 ? s->d_dchunk : s->d_dchunk2, R == 1 ? s->ndchunk : s->ndchunk2,
                     s->d_dops, s->d_rank16, s->d_pat16, s->d_map, s->T.ns, (const V*)x, s->dim, s->row0, epi);
  return ED_OK;
}

template <bool HC, bool VC, int CPT, int DEGU, int RU>
static int launch_kron_up_t(ed_sector* s, const void* x, void* y, hipStream_t st, int64_t w0, int64_t nw) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  KronHost& K = s->K;
  const size_t lds = kron_up_lds(HC, VC, K.dimup, RU);
  auto fn = k_kron_up<HC, VC, CPT, DEGU, RU>;
  static thread_local int attr_set = 0;
  if (!attr_set) {
    HIPCK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = 1;
  }
  static thread_local int up_grid = 0;  // per instantiation and LDS size (occupancy x CUs)
  static thread_local size_t up_lds = 0;
  if (!up_grid || up_lds != lds) {
    up_lds = lds;
    int per = 0, dev = 0, ncu = 0;
    HIPCK(hipGetDevice(&dev));
    HIPCK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)fn, kKronUpBlock, lds));
    up_grid = std::max(per, 1) * ncu;
  }
  // down rows [w0, w0+nw) (the whole sector, or a rank's row block: x, y
  // are then that block)
  KronArgs<HC> ka = kron_args<HC>(s);
  ka.adw += w0;
  ka.impd += w0;
  ka.dimdw = nw;
  hipLaunchKernelGGL(fn, dim3((int)std::min<int64_t>(nw, up_grid)), dim3(kKronUpBlock), lds, st, ka, K.upw,
                     (const H*)K.updict, K.nupdict, (const V*)x, (V*)y);
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool HC, bool VC, int CPT, int DEGU>
static int launch_kron_up(ed_sector* s, const void* x, void* y, hipStream_t st, int64_t w0, int64_t nw) {
  // two staged rows per step when LDS allows, except at 4 columns x > 8 slots
  // per thread, where the second row's registers spill (n28b pass U: 97 us
  // with 2 rows, 67 us with 1)
  if (!(CPT >= 4 && DEGU > 8) && kron_up_rows(HC, VC, s->K.dimup) == 2)
    return launch_kron_up_t<HC, VC, CPT, DEGU, 2>(s, x, y, st, w0, nw);
  return launch_kron_up_t<HC, VC, CPT, DEGU, 1>(s, x, y, st, w0, nw);
}

// pass U over down rows [w0, w0+nw)
template <bool HC, bool VC>
static int launch_kron_up_any(ed_sector* s, const void* x, void* y, hipStream_t st, int64_t w0, int64_t nw) {
  switch (s->K.cpt * 100 + s->K.degU) {
    case 108: return launch_kron_up<HC, VC, 1, 8>(s, x, y, st, w0, nw);
    case 116: return launch_kron_up<HC, VC, 1, 16>(s, x, y, st, w0, nw);
    case 208: return launch_kron_up<HC, VC, 2, 8>(s, x, y, st, w0, nw);
    case 112: return launch_kron_up<HC, VC, 1, 12>(s, x, y, st, w0, nw);
    case 212: return launch_kron_up<HC, VC, 2, 12>(s, x, y, st, w0, nw);
    case 216: return launch_kron_up<HC, VC, 2, 16>(s, x, y, st, w0, nw);
    case 408: return launch_kron_up<HC, VC, 4, 8>(s, x, y, st, w0, nw);
    case 412: return launch_kron_up<HC, VC, 4, 12>(s, x, y, st, w0, nw);
    case 808: return launch_kron_up<HC, VC, 8, 8>(s, x, y, st, w0, nw);
    default: return fail(ED_ERR_STATE, "kron2: no instantiation for this geometry");
  }
}

// pass D with rows of length ld over columns [0, ncols); ypart may be null
template <bool HC, bool VC, class Epi>
static int launch_kron_dw(ed_sector* s, const void* x, const void* ypart, Epi epi, hipStream_t st, int ld,
                          int ncols) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  KronHost& K = s->K;
  const int grid = kron_dw_grid(s, VC);
  if constexpr (!HC && !VC) {
    // two columns per lane (16-byte gathers) where the rows, the column
    // range, both vectors and (plain store: one 16-byte store per lane) the
    // output are 16-byte aligned
    bool a16 = ((uintptr_t)x % 16) == 0 && ((uintptr_t)ypart % 16) == 0;
    if constexpr (std::is_same_v<Epi, EpiStore<VC>>) a16 = a16 && ((uintptr_t)epi.hv % 16) == 0;
    if (ld % 2 == 0 && ncols % 2 == 0 && a16) {
      if (K.degD == 8)
        hipLaunchKernelGGL((k_kron_dw<HC, VC, 8, Epi, 2>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                           K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld,
                           ncols);
      else if (K.degD == 12)
        hipLaunchKernelGGL((k_kron_dw<HC, VC, 12, Epi, 2>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                           K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld,
                           ncols);
      else
        hipLaunchKernelGGL((k_kron_dw<HC, VC, 16, Epi, 2>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                           K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld,
                           ncols);
      HIPCK(hipGetLastError());
      return ED_OK;
    }
  }
  if (K.degD == 8)
    hipLaunchKernelGGL((k_kron_dw<HC, VC, 8, Epi>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                       K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld, ncols);
  else if (K.degD == 12)
    hipLaunchKernelGGL((k_kron_dw<HC, VC, 12, Epi>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                       K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld, ncols);
  else
    hipLaunchKernelGGL((k_kron_dw<HC, VC, 16, Epi>), dim3(grid), dim3(kBlock), 0, st, kron_args<HC>(s),
                       K.dwo, K.dwi, (const H*)K.dwdict, K.ndwdict, (const V*)x, (const V*)ypart, epi, ld, ncols);
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool HC, bool VC, class Epi>
static int launch_kron2(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  void* y = (void*)epi.scratch();
  CK((launch_kron_up_any<HC, VC>(s, x, y, st, 0, s->K.dimdw)));
  return launch_kron_dw<HC, VC>(s, x, y, epi, st, (int)s->K.dimup, (int)s->K.dimup);
}

// Two-segment stored H·v (ed_split.hpp): segment A (diagonal + in-block
// elements, k_spmv_pk on the A words) writes y into the epilogue's scratch
// vector, segment B adds the cross-block elements and runs the epilogue.
template <bool HC, bool VC, class Epi>
static int launch_split(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  if constexpr (HC || VC) {
    // (split_on(): real H on real vectors only; the complex forms are not instantiated)
    return fail(ED_ERR_STATE, "two-segment stored H·v serves real H on real vectors");
  } else {
    V* y = (V*)epi.scratch();
    const int64_t dim = s->dim, ns = s->nslice;
    const bool nta = (s->paddedA * 4 + dim * (int64_t)sizeof(H)) > kSplitMinBytes;
    // A: rows of exactly 7 in-block elements (Norb=1, Nbath=13 half filling)
    // take 7-slot chunks, rows of <= 8 chunks of 8 slots (fewer padding
    // gathers than 16); two slices per wave
#define ED_SPA(NTV, CH)                                                                                       \
  hipLaunchKernelGGL((k_spmv_sa<HC, VC, NTV, CH, ED_SA_R>),                                                    \
                     dim3(resident_grid((const void*)k_spmv_sa<HC, VC, NTV, CH, ED_SA_R>, kBlock)), dim3(kBlock), 0, st, \
                     (const H*)s->d_diag, s->d_sptrA, s->d_wordsA, (const H*)s->d_pdict, (const V*)x, y, dim, ns)
    if (s->wA_max == 7 && s->wA_min == 7) {
      if (nta) ED_SPA(1, 7);
      else ED_SPA(0, 7);
    } else if (s->wA_max <= 8) {
      if (nta) ED_SPA(1, 8);
      else ED_SPA(0, 8);
    } else if (s->wA_max <= 12) {  // (Norb=2: up to 12 in-block elements per row)
      if (nta) ED_SPA(1, 12);
      else ED_SPA(0, 12);
    } else {
      if (nta) ED_SPA(1, kChunk);
      else ED_SPA(0, kChunk);
    }
#undef ED_SPA
    HIPCK(hipGetLastError());
#define ED_SPB(NTV, U)                                                                                        \
  hipLaunchKernelGGL((k_spmv_sb<HC, VC, NTV, Epi, U>), dim3(kSplitGrid), dim3(kBlock), 0, st, s->d_bsl, s->d_itR, \
                     s->d_xoff, s->d_glist, s->d_xoff + 9, s->d_ul, s->d_lw, (const H*)s->d_pdict, (const V*)x,   \
                     (const V*)y, epi)
    const bool ntb = s->nlw * 4 > kSplitMinBytes;
    if (s->split_uch == 7) {
      if (ntb) ED_SPB(1, 7);
      else ED_SPB(0, 7);
    } else {
      if (ntb) ED_SPB(1, kSplitChunk);
      else ED_SPB(0, kSplitChunk);
    }
#undef ED_SPB
    HIPCK(hipGetLastError());
    return ED_OK;
  }
}

// Fused one-pass re-laid stored H·v (ed_fused.hpp).  Grid: half the
// resident blocks, a multiple of 8 (one unit range per XCD) — 16 waves per
// CU keep the window of units an XCD works on (and the neighbour V rows its
// cross-block gathers read) smaller than the full resident grid does: N28
// complex H 0.281 -> 0.269 ms, complex vectors on real H 0.275 -> 0.262, N28
// Jx/Jp real 0.239 -> 0.228; a quarter measured slower (gpurun_out r6f)
#ifndef ED_FU_GRID_DIV
#define ED_FU_GRID_DIV 2
#endif
int fused_grid(const ed_sector* s, int vc) {
  const int g = vc ? resident_grid((const void*)k_spmv_fu<false, true, 1, EpiStore<true>, 8, 8>, kBlock)
                   : resident_grid((const void*)k_spmv_fu<false, false, 1, EpiStore<false>, 8, 8>, kBlock);
  (void)s;
  return std::max(8, (g / ED_FU_GRID_DIV) & ~7);
}

template <bool HC, bool VC, class Epi>
static int launch_fused(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  const int g = fused_grid(s, VC);
  const bool nt = (s->fu_na + s->fu_nl) * 4 + s->dim * (int64_t)sizeof(H) > kSplitMinBytes;
#define ED_FU(NTV, CH, U)                                                                                      \
  hipLaunchKernelGGL((k_spmv_fu<HC, VC, NTV, Epi, CH, U>), dim3(g), dim3(kBlock), 0, st, (const H*)s->d_diag,      \
                     s->d_fu, s->nfu, s->d_fa, s->d_ful, s->d_flw, (const H*)s->d_pdict, (const V*)x, epi)
#define ED_FU_CH(NTV, U)                                                   \
  do {                                                                     \
    if (s->fu_wa_max == 7 && s->fu_wa_min == 7) ED_FU(NTV, 7, U);          \
    else if (s->fu_wa_max <= 8 || kFuChMax <= 8) ED_FU(NTV, 8, U);         \
    else if (s->fu_wa_max <= 12 || kFuChMax <= 12) ED_FU(NTV, 12, U);      \
    else ED_FU(NTV, kChunk, U);                                            \
  } while (0)
  if (s->fu_uch == 7) {
    if (nt) ED_FU_CH(1, 7);
    else ED_FU_CH(0, 7);
  } else {
    if (nt) ED_FU_CH(1, kFuUChunk);
    else ED_FU_CH(0, kFuUChunk);
  }
#undef ED_FU_CH
#undef ED_FU
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool HC, bool VC, class Epi>
static int launch_hxv_t(ed_sector* s, int path, const void* x, Epi epi, hipStream_t st) {
  using V = val_t<VC>;
  const int64_t dim = s->nrows, ns = s->nslice;  // rows of this object; x is the whole sector vector
  const int g = grid_for(ns * 64);
  const int gx = hxv_blocks(s, path, VC);
  const int xr = xcd_on(s, path) ? 1 : 0;
  const V* xo = (const V*)x + s->row0;  // the rows' own entries
  // non-temporal matrix loads once the matrix cannot stay in the 256 MB MALL
  const bool nt = stored_mbytes(s) > ((int64_t)192 << 20);
  // (segment B's pair items load x and y and store the plain epilogue's Hv
  // = y 16 bytes at a time: an 8-byte aligned view, e.g. a torch slice at an
  // odd offset, takes the one-pass kernel)
  if (fused_on(s, path, VC)) return launch_fused<HC, VC>(s, x, epi, st);
  if (split_on(s, path, VC) && !(((uintptr_t)x | (uintptr_t)epi.scratch()) & 15))
    return launch_split<HC, VC>(s, x, epi, st);
  if (path == 0 && s->d_words) {
    using H = val_t<HC>;
    if (nt)
      hipLaunchKernelGGL((k_spmv_pk<HC, VC, 1, Epi>), dim3(gx), dim3(kBlock), 0, st, (const H*)s->d_diag,
                         s->d_sptr, s->d_words, (const H*)s->d_pdict, (const V*)x, xo, dim, ns, epi, xr);
    else
      hipLaunchKernelGGL((k_spmv_pk<HC, VC, 0, Epi>), dim3(gx), dim3(kBlock), 0, st, (const H*)s->d_diag,
                         s->d_sptr, s->d_words, (const H*)s->d_pdict, (const V*)x, xo, dim, ns, epi, xr);
  } else if (path == 0) {
    if (nt)
      hipLaunchKernelGGL((k_spmv<HC, VC, 1, Epi>), dim3(gx), dim3(kBlock), 0, st,
                         (const val_t<HC>*)s->d_diag, s->d_sptr, s->d_cols,
                         (const val_t<HC>*)s->d_vals, (const V*)x, xo, dim, ns, epi, xr);
    else
      hipLaunchKernelGGL((k_spmv<HC, VC, 0, Epi>), dim3(gx), dim3(kBlock), 0, st,
                         (const val_t<HC>*)s->d_diag, s->d_sptr, s->d_cols,
                         (const val_t<HC>*)s->d_vals, (const V*)x, xo, dim, ns, epi, xr);
  } else if (path == 1) {
    const int rc = s->dir_patlds ? launch_direct<HC, VC, true>(s, x, epi, st)
                                 : launch_direct<HC, VC, false>(s, x, epi, st);
    if (rc != ED_OK) return rc;
  } else if (kron2_on(s, path, VC)) {
    return launch_kron2<HC, VC>(s, x, epi, st);
  } else {
    hipLaunchKernelGGL((k_kron<HC, VC, Epi>), dim3(g), dim3(kBlock), 0, st, kron_args<HC>(s),
                       (const V*)x, dim, ns, epi);
  }
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool VC, class Epi>
int launch_hxv(ed_sector* s, int path, const void* x, Epi epi, hipStream_t st) {
  if (s->hc) {
    if constexpr (VC) return launch_hxv_t<true, true>(s, path, x, epi, st);
    return fail(ED_ERR_ARG, "complex Hamiltonian needs complex vectors (vtype=1)");
  }
  return launch_hxv_t<false, VC>(s, path, x, epi, st);
}

// launch_hxv's instantiations (declared in ed_sector.hpp): every H·v kernel
// of the library is compiled here, once
#define ED_HXV_INST(VC, EPI) \
  template int launch_hxv<VC, EPI<VC>>(ed_sector*, int, const void*, EPI<VC>, hipStream_t);
ED_HXV_INST(false, EpiStore) ED_HXV_INST(true, EpiStore)
ED_HXV_INST(false, EpiTrlLoc) ED_HXV_INST(true, EpiTrlLoc)
ED_HXV_INST(false, EpiLancA) ED_HXV_INST(true, EpiLancA)
#undef ED_HXV_INST

template <bool HC, bool VC>
static int kron_split_launch(ed_sector* s, int part, int64_t o, int64_t n, const void* x, void* y, int acc,
                             hipStream_t st) {
  using V = val_t<VC>;
  const int64_t cnt = n * (part == 0 ? s->K.dimup : s->K.dimdw);
  if (cnt == 0) return ED_OK;
  // the two-pass kernels serve the split too (pass U on the row block, pass D
  // on the column strip, ld = nu): same products, same order as
  // k_kron_rows / k_kron_cols
  if (kron2_on(s, 2, VC) && !(s->opts & ED_OPT_SPLIT_SIMPLE)) {
    if (part == 0) return launch_kron_up_any<HC, VC>(s, x, y, st, o, n);
    EpiStore<VC> e{(V*)y};
    return launch_kron_dw<HC, VC>(s, x, acc ? y : nullptr, e, st, (int)n, (int)n);
  }
  if (part == 0)
    hipLaunchKernelGGL((k_kron_rows<HC, VC>), dim3(grid_for(cnt)), dim3(kBlock), 0, st, kron_args<HC>(s), o, n,
                       (const V*)x, (V*)y);
  else
    hipLaunchKernelGGL((k_kron_cols<HC, VC>), dim3(grid_for(cnt)), dim3(kBlock), 0, st, kron_args<HC>(s), n,
                       (const V*)x, (V*)y, acc);
  HIPCK(hipGetLastError());
  return ED_OK;
}

static int kron_split(ed_sector* s, int part, int32_t vtype, int64_t o, int64_t n, const void* x, void* y,
                      int acc, void* stream) {
  if (!s || !x || !y) return fail(ED_ERR_ARG, "null");
  if (!s->kron) return fail(ED_ERR_UNSUPPORTED, "sector has no Kronecker form (normal mode without Jx/Jp, ED_DIRECT)");
  const int64_t lim = part == 0 ? s->K.dimdw : s->K.dimup;
  if (o < 0 || n < 0 || o + n > lim) return fail(ED_ERR_ARG, "row/column range outside the factor dimension");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  if (vtype == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (s->hc) return kron_split_launch<true, true>(s, part, o, n, x, y, acc, st);
  return vtype ? kron_split_launch<false, true>(s, part, o, n, x, y, acc, st)
               : kron_split_launch<false, false>(s, part, o, n, x, y, acc, st);
}

extern "C" {

int ed_sector_hxv_dev_path(ed_sector* s, int32_t path, int32_t vtype, const void* v, void* hv,
                           void* stream) {
  if (s && s->nrows == 0) return ED_OK;  // no local rows: nothing to write
  if (!s || !v || !hv) return fail(ED_ERR_ARG, "null");
  int pth = resolve_path(s, path);
  if (pth < 0) return fail(ED_ERR_ARG, "H·v path not available for this sector");
  HIPCK(hipSetDevice(s->device));
  CK(ensure_direct(s, pth, (hipStream_t)stream));
  hipStream_t st = (hipStream_t)stream;
  if (vtype == 1) {
    EpiStore<true> e{(double2*)hv};
    return launch_hxv<true>(s, pth, v, e, st);
  }
  if (vtype == 0) {
    EpiStore<false> e{(double*)hv};
    return launch_hxv<false>(s, pth, v, e, st);
  }
  return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
}

int ed_sector_col_mask(const ed_sector* s, uint32_t* mask_dev, void* stream) {
  if (!s || !mask_dev) return fail(ED_ERR_ARG, "null");
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  HIPCK(hipMemsetAsync(mask_dev, 0, (size_t)((s->dim + 31) / 32) * 4, st));
  if (s->nrows == 0) return ED_OK;
  DevIndex idx{s->d_off, s->d_rank, s->T.ns, s->T.nst - 1};
  hipLaunchKernelGGL(k_mark_cols, dim3(grid_for(s->nrows)), dim3(kBlock), 0, st, s->Md, s->d_map + s->row0,
                     s->nrows, idx, mask_dev);
  HIPCK(hipGetLastError());
  return ED_OK;
}

int ed_sector_kron_rows(ed_sector* s, int32_t vtype, int64_t w0, int64_t nw, const void* x, void* y,
                        void* stream) {
  return kron_split(s, 0, vtype, w0, nw, x, y, 0, stream);
}

int ed_sector_kron_cols(ed_sector* s, int32_t vtype, int64_t u0, int64_t nu, const void* xt, void* yt,
                        int32_t accumulate, void* stream) {
  return kron_split(s, 1, vtype, u0, nu, xt, yt, accumulate, stream);
}

int ed_sector_hxv_dev(ed_sector* s, int32_t vtype, const void* v, void* hv, void* stream) {
  return ed_sector_hxv_dev_path(s, -1, vtype, v, hv, stream);
}

int ed_sector_hxv(ed_sector* s, int32_t nloc, const double* v, double* hv) {
  if (!s || !v || !hv) return fail(ED_ERR_ARG, "null");
  CK(whole_only(s));
  // directMatVec_cc: "Nloc != dim(isector)" (DIRECT_HxV.f90:50)
  if ((int64_t)nloc != s->dim) return fail(ED_ERR_ARG, "ed_gpu_hxv ERROR: Nloc != dim(isector)");
  HIPCK(hipSetDevice(s->device));
  if (!s->d_x) {
    CK(dalloc(s, &s->d_x, s->dim * 16));
    CK(dalloc(s, &s->d_y, s->dim * 16));
  }
  HIPCK(hipMemcpyAsync(s->d_x, v, s->dim * 16, hipMemcpyHostToDevice, s->stream));
  CK(ed_sector_hxv_dev(s, 1, s->d_x, s->d_y, s->stream));
  HIPCK(hipMemcpyAsync(hv, s->d_y, s->dim * 16, hipMemcpyDeviceToHost, s->stream));
  HIPCK(hipStreamSynchronize(s->stream));
  return ED_OK;
}


// what ed_seed_plan.hpp needs to know of a (src, dst) pair
static SeedSectors seed_sectors(const ed_sector* src, const ed_sector* dst) {
  return SeedSectors{src->Mh.ns, src->Mh.mode, src->Mh.jz, src->Mh.lz2,
                     (int32_t)src->T.q1, (int32_t)src->T.q2, (int32_t)dst->T.q1, (int32_t)dst->T.q2};
}

// dst must be exactly the sector the operator maps src into (getCsector /
// getCDGsector, ED_SETUP.f90:464-495, 590-619, 750-768); otherwise targets
// would fall outside dst's index tables
static int check_op_target(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t level) {
  if (!src || !dst) return fail(ED_ERR_ARG, "null");
  if (src->device != dst->device) return fail(ED_ERR_ARG, "sectors on different devices");
  if (op != 0 && op != 1) return fail(ED_ERR_ARG, "op must be 0 (c) or 1 (c^+)");
  if (level < 0 || level >= 2 * src->Mh.ns || src->Mh.ns != dst->Mh.ns)
    return fail(ED_ERR_ARG, "level outside the 2*Ns Fock levels / mismatched models");
  // the sector arithmetic is seed_op_target's (ed_seed_plan.hpp), one definition
  int32_t e1, e2;
  if (seed_op_target(seed_sectors(src, dst), op, level, &e1, &e2) != ED_OK)
    return fail(ED_ERR_ARG, "unknown ed_mode");
  if (dst->Mh.mode != src->Mh.mode || dst->Mh.jz != src->Mh.jz || dst->T.q1 != e1 || dst->T.q2 != e2)
    return fail(ED_ERR_ARG, "dst is not the sector reached by the operator");
  return ED_OK;
}

int ed_sector_apply_op(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t level,
                       int32_t vtype, const void* src_vec, void* dst_vec, void* stream) {
  if (!src_vec || !dst_vec) return fail(ED_ERR_ARG, "null");
  CK(check_op_target(src, dst, op, level));
  CK(whole_only(src));
  CK(whole_only(dst));
  HIPCK(hipSetDevice(src->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t vs = vtype ? 16 : 8;
  HIPCK(hipMemsetAsync(dst_vec, 0, dst->dim * vs, st));
  DevIndex idx{dst->d_off, dst->d_rank, dst->T.ns, dst->T.nst - 1};
  if (vtype)
    hipLaunchKernelGGL(k_apply_op<true>, dim3(grid_for(src->dim)), dim3(kBlock), 0, st, src->d_map,
                       src->dim, idx, op, level, (const double2*)src_vec, (double2*)dst_vec);
  else
    hipLaunchKernelGGL(k_apply_op<false>, dim3(grid_for(src->dim)), dim3(kBlock), 0, st, src->d_map,
                       src->dim, idx, op, level, (const double*)src_vec, (double*)dst_vec);
  HIPCK(hipGetLastError());
  return ED_OK;
}

int ed_sector_apply_op_acc(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t level,
                           double coef_re, double coef_im, int32_t vtype, const void* src_vec,
                           void* dst_vec, void* stream) {
  if (!src_vec || !dst_vec) return fail(ED_ERR_ARG, "null");
  if (!vtype && coef_im != 0.0) return fail(ED_ERR_ARG, "complex coefficient needs vtype=1");
  CK(whole_only(src));
  CK(whole_only(dst));
  CK(check_op_target(src, dst, op, level));
  HIPCK(hipSetDevice(src->device));
  hipStream_t st = (hipStream_t)stream;
  DevIndex idx{dst->d_off, dst->d_rank, dst->T.ns, dst->T.nst - 1};
  if (vtype)
    hipLaunchKernelGGL(k_apply_op_acc<true>, dim3(grid_for(src->dim)), dim3(kBlock), 0, st,
                       src->d_map, src->dim, idx, op, level, coef_re, coef_im,
                       (const double2*)src_vec, (double2*)dst_vec);
  else
    hipLaunchKernelGGL(k_apply_op_acc<false>, dim3(grid_for(src->dim)), dim3(kBlock), 0, st,
                       src->d_map, src->dim, idx, op, level, coef_re, coef_im,
                       (const double*)src_vec, (double*)dst_vec);
  HIPCK(hipGetLastError());
  return ED_OK;
}

// ------------------------------------------------ fused seeds (ed_seed.hpp, ed_chi.hpp)
// The seed pipeline, one for the four entries below: the entry validates its
// own table or plan, seed_check_io checks what they share, and seed_run
// launches the entry's gather kernel, k_seed_scale and the download of the
// norms.  Every check comes before the first launch: a refused call leaves
// `seeds` untouched.
static constexpr int kSeedMaxGrid = 1024;  // partials per seed: the cap kObsMaxGrid puts on the observables' grids

// The kernel arguments keep their sizes: the kernels are compiled for these.
static_assert(sizeof(SeedPlan) == 84 && sizeof(PairPlan) == 80 && sizeof(SeedTable) == 3136 &&
                  sizeof(DiagTable) == 1568,
              "a seed kernel's argument changed size");

static bool same_model(const EdModel& a, const EdModel& b) {
  return a.ns == b.ns && a.norb == b.norb && a.nbath == b.nbath && a.nspin == b.nspin && a.mode == b.mode &&
         a.bath == b.bath && a.jz == b.jz;
}

// src_vec: [src->dim] read by the gather; seeds: [nseed][dst->dim] written by
// it.  The gather kernels read x[idx_src(s)] while other threads store whole
// output rows, so the two may not overlap.  src == dst is allowed.
static int seed_check_io(const ed_sector* src, const ed_sector* dst, int32_t nseed, int32_t vtype,
                         const void* src_vec, const void* seeds) {
  if (!src || !dst || !src_vec || !seeds) return fail(ED_ERR_ARG, "null");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  if (src->device != dst->device) return fail(ED_ERR_ARG, "sectors on different devices");
  if (!same_model(src->Mh, dst->Mh)) return fail(ED_ERR_ARG, "sectors of different models");
  CK(whole_only(src));
  CK(whole_only(dst));
  const size_t vs = vtype ? 16 : 8;
  const uintptr_t a = (uintptr_t)src_vec, b = (uintptr_t)seeds;
  if (a < b + (size_t)nseed * dst->dim * vs && b < a + (size_t)src->dim * vs)
    return fail(ED_ERR_ARG, "seeds overlaps src_vec");
  return ED_OK;
}

// launch_gather(vc_tag, g, partials, st) issues the entry's gather kernel with
// grid g on st: it leaves the unnormalised seeds [nseed][dst->dim] and one
// partial of sum |seed_q|^2 per seed and block.  vc_tag is
// std::bool_constant<VC>, VC the kernel's vector type.
extern "C++" template <class Launch>
static int seed_run(const ed_sector* dst, int32_t nseed, int32_t vtype, void* seeds, double* norm2, void* stream,
                    Launch launch_gather) {
  HIPCK(hipSetDevice(dst->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t dim = dst->dim;
  const int g = std::min(grid_for(dim), kSeedMaxGrid);
  double* part = nullptr;  // partials [nseed][g] | norm2 [nseed]
  HIPCK(hipMallocAsync((void**)&part, ((size_t)nseed * g + nseed) * sizeof(double), st));
  DevFree fr{part, st};
  PinnedLease pin((size_t)nseed * sizeof(double), st);
  if (!pin.p) return fail(ED_ERR_OOM, "pinned staging");
  double* dn = part + (size_t)nseed * g;
  double* hn = (double*)pin.p;
  if (vtype) {
    launch_gather(std::true_type{}, g, part, st);
    HIPCK(hipGetLastError());
    hipLaunchKernelGGL(k_seed_scale<true>, dim3(g, nseed), dim3(kBlock), 0, st, (double2*)seeds, dim, part, g, dn);
  } else {
    launch_gather(std::false_type{}, g, part, st);
    HIPCK(hipGetLastError());
    hipLaunchKernelGGL(k_seed_scale<false>, dim3(g, nseed), dim3(kBlock), 0, st, (double*)seeds, dim, part, g, dn);
  }
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(hn, dn, (size_t)nseed * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  memcpy(norm2, hn, (size_t)nseed * sizeof(double));
  return ED_OK;
}

// Every seed of one (source vector, operator type, target sector) group: the
// vvinit loops ED_GF_NORMAL.f90:159-174 and :312-344 with their dot_product
// and divide, as one gather pass over dst's rows and one scale pass.
int ed_sector_seed_batch(const ed_sector* src, const ed_sector* dst, int32_t op, int32_t nlev,
                         const int32_t* levels, int32_t nseed, const double* coef, int32_t vtype,
                         const void* src_vec, void* seeds, double* norm2, void* stream) {
  if (!levels || !coef || !norm2) return fail(ED_ERR_ARG, "null");
  if (nlev < 1 || nlev > kSeedMaxLev) return fail(ED_ERR_ARG, "nlev must be 1..2*ED_MAX_NORB");
  if (nseed < 1 || nseed > kSeedMaxSeeds) return fail(ED_ERR_ARG, "nseed must be 1..32");
  CK(seed_check_io(src, dst, nseed, vtype, src_vec, seeds));
  SeedTable T{};
  T.nlev = nlev;
  T.nseed = nseed;
  for (int l = 0; l < nlev; l++) {
    // the kernel's index tables do not bounds-check: every level must map src into dst
    CK(check_op_target(src, dst, op, levels[l]));
    for (int k = 0; k < l; k++)
      if (levels[k] == levels[l]) return fail(ED_ERR_ARG, "levels must be distinct");
    T.lev[l] = levels[l];
  }
  for (int q = 0; q < nseed; q++)
    for (int l = 0; l < nlev; l++) {
      T.cr[q][l] = coef[2 * ((size_t)q * nlev + l)];
      T.ci[q][l] = coef[2 * ((size_t)q * nlev + l) + 1];
      if (!vtype && T.ci[q][l] != 0.0) return fail(ED_ERR_ARG, "complex coefficient needs vtype=1");
      if (T.cr[q][l] != 0.0 || T.ci[q][l] != 0.0) T.used[q] |= (uint8_t)(1u << l);
    }
  const DevIndex idx{src->d_off, src->d_rank, src->T.ns, src->T.nst - 1};
  return seed_run(dst, nseed, vtype, seeds, norm2, stream, [&](auto vc, int g, double* part, hipStream_t st) {
    constexpr bool VC = decltype(vc)::value;
    hipLaunchKernelGGL(k_seed_gather<VC>, dim3(g), dim3(kBlock), 0, st, dst->d_map, dst->dim, idx, op, T,
                       (const val_t<VC>*)src_vec, (val_t<VC>*)seeds, part);
  });
}

// Seeds whose images mix operator types: the six vvinit loops of
// lanc_build_gf_superc_c (ED_GF_SUPERC.f90:119-439) per kept state, three per
// target sector, with their dot_product and divide.  seed_plan_compile checks
// that every image maps src into dst.
int ed_sector_seed_plan(const ed_sector* src, const ed_sector* dst, int32_t nlev, const int32_t* levels,
                        const int32_t* ops, int32_t nseed, const int32_t* terms, int32_t vtype,
                        const void* src_vec, void* seeds, double* norm2, void* stream) {
  if (!levels || !ops || !terms || !norm2) return fail(ED_ERR_ARG, "null");
  if (nlev < 1 || nlev > kSeedMaxLev) return fail(ED_ERR_ARG, "nlev must be 1..2*ED_MAX_NORB");
  if (nseed < 1 || nseed > kSeedMaxSeeds) return fail(ED_ERR_ARG, "nseed must be 1..32");
  CK(seed_check_io(src, dst, nseed, vtype, src_vec, seeds));
  SeedPlan P;
  if (seed_plan_compile(seed_sectors(src, dst), nlev, levels, ops, nseed, terms, &P) != ED_OK)
    return fail(ED_ERR_ARG, "seed plan: every image maps src into dst, (level, op) pairs must be distinct, "
                            "p and q below nlev, p != q");
  const DevIndex idx{src->d_off, src->d_rank, src->T.ns, src->T.nst - 1};
  return seed_run(dst, nseed, vtype, seeds, norm2, stream, [&](auto vc, int g, double* part, hipStream_t st) {
    constexpr bool VC = decltype(vc)::value;
    hipLaunchKernelGGL(k_seed_plan<VC>, dim3(g), dim3(kBlock), 0, st, dst->d_map, dst->dim, idx, P,
                       (const val_t<VC>*)src_vec, (val_t<VC>*)seeds, part);
  });
}

// Seeds of operators diagonal in the Fock basis (ed_chi.hpp): the vvinit loops
// of lanc_ed_build_spinChi_c (ED_GF_CHISPIN.f90:98-103), _tot_c
// (ED_GF_CHISPIN.f90:194-199) and of the density builders
// (ED_GF_CHIDENS.f90:127-132) for every operator of one kept state, with their
// dot_product and divide.  The seed stays in s.
int ed_sector_seed_diag(const ed_sector* s, int32_t nlev, const int32_t* levels, int32_t nseed,
                        const double* weight, int32_t vtype, const void* src_vec, void* seeds, double* norm2,
                        void* stream) {
  if (!levels || !weight || !norm2) return fail(ED_ERR_ARG, "null");
  if (nlev < 1 || nlev > kDiagMaxLev) return fail(ED_ERR_ARG, "nlev must be 1..2*ED_MAX_NORB");
  if (nseed < 1 || nseed > kDiagMaxSeeds) return fail(ED_ERR_ARG, "nseed must be 1..32");
  CK(seed_check_io(s, s, nseed, vtype, src_vec, seeds));
  DiagTable T;
  if (seed_diag_compile(s->Mh.ns, nlev, levels, nseed, weight, &T) != ED_OK)
    return fail(ED_ERR_ARG, "seed table: levels must be distinct and below 2*Ns");
  return seed_run(s, nseed, vtype, seeds, norm2, stream, [&](auto vc, int g, double* part, hipStream_t st) {
    constexpr bool VC = decltype(vc)::value;
    hipLaunchKernelGGL(k_seed_diag<VC>, dim3(g), dim3(kBlock), 0, st, s->d_map, s->dim, T,
                       (const val_t<VC>*)src_vec, (val_t<VC>*)seeds, part);
  });
}

// Seeds whose images are products of two ladder operators (ed_chi.hpp,
// ed_seed_pair.hpp): the vvinit loops of the pair susceptibility
// (ED_GF_CHIPAIR.f90:98-102, :144-148) and of lanc_ed_build_densChi_mix_c
// (ED_GF_CHIDENS.f90:523-586, :596-659) for every operator of one kept state,
// with their dot_product and divide.  src == dst is allowed (the inter-orbital
// seeds stay in the kept state's sector).  seed_pair_compile checks that every
// image maps src into dst.
int ed_sector_seed_pair(const ed_sector* src, const ed_sector* dst, int32_t nimg, const int32_t* images,
                        int32_t nseed, const int32_t* terms, int32_t vtype, const void* src_vec, void* seeds,
                        double* norm2, void* stream) {
  if (!images || !terms || !norm2) return fail(ED_ERR_ARG, "null");
  if (nimg < 1 || nimg > kPairMaxImg) return fail(ED_ERR_ARG, "nimg must be 1..12");
  if (nseed < 1 || nseed > kPairMaxSeeds) return fail(ED_ERR_ARG, "nseed must be 1..12");
  CK(seed_check_io(src, dst, nseed, vtype, src_vec, seeds));
  PairPlan P;
  if (seed_pair_compile(seed_sectors(src, dst), nimg, images, nseed, terms, &P) != ED_OK)
    return fail(ED_ERR_ARG, "seed pair plan: lev1 != lev2, every image maps src into dst, images distinct, "
                            "p and q below nimg, p != q");
  const DevIndex idx{src->d_off, src->d_rank, src->T.ns, src->T.nst - 1};
  return seed_run(dst, nseed, vtype, seeds, norm2, stream, [&](auto vc, int g, double* part, hipStream_t st) {
    constexpr bool VC = decltype(vc)::value;
    hipLaunchKernelGGL(k_seed_pair<VC>, dim3(g), dim3(kBlock), 0, st, dst->d_map, dst->dim, idx, P,
                       (const val_t<VC>*)src_vec, (val_t<VC>*)seeds, part);
  });
}

// ------------------------------------------------ twin-sector vectors
// (ed_twin.hpp).  get_twin_sector (ED_SETUP.f90:1196-1212): (nup, ndw) ->
// (ndw, nup), sz -> -sz, n -> 2*Ns - n; it knows no (n, twoJz) sectors.
static int check_twin_pair(const ed_sector* src, const ed_sector* dst) {
  if (!src || !dst) return fail(ED_ERR_ARG, "null");
  if (src->device != dst->device) return fail(ED_ERR_ARG, "sectors on different devices");
  const EdModel& a = src->Mh;
  if (!same_model(a, dst->Mh)) return fail(ED_ERR_ARG, "sectors of different models");
  if (a.jz) return fail(ED_ERR_ARG, "twin sectors are not defined in the Jz basis");
  int e1, e2 = 0;
  if (a.mode == ED_MODE_NORMAL) {
    e1 = src->T.q2;
    e2 = src->T.q1;
  } else if (a.mode == ED_MODE_SUPERC) {
    e1 = -src->T.q1;
  } else {
    e1 = 2 * a.ns - src->T.q1;
  }
  if (dst->T.q1 != e1 || (a.mode == ED_MODE_NORMAL && dst->T.q2 != e2) || dst->dim != src->dim)
    return fail(ED_ERR_ARG, "dst is not the twin sector of src");
  return ED_OK;
}

int ed_sector_twin_vector(const ed_sector* src, const ed_sector* dst, int32_t vtype, const void* src_vec,
                          void* dst_vec, void* stream) {
  if (!src_vec || !dst_vec || src_vec == dst_vec) return fail(ED_ERR_ARG, "null or aliased vectors");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  CK(check_twin_pair(src, dst));
  CK(whole_only(src));
  CK(whole_only(dst));
  HIPCK(hipSetDevice(src->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t dim = dst->dim;
  if (src->Mh.mode == ED_MODE_NORMAL && !(dst->opts & ED_OPT_TWIN_GATHER)) {
    const int64_t R = src->T.dimdw, C = src->T.dimup;  // the partner's view: idw rows, iup fast
    const int64_t nt = ((R + kTwinTile - 1) / kTwinTile) * ((C + kTwinTile - 1) / kTwinTile);
    const int g = (int)std::min<int64_t>(nt, 8 * 256);
    if (vtype)
      hipLaunchKernelGGL(k_twin_transpose<true>, dim3(g), dim3(kBlock), 0, st, R, C, (const double2*)src_vec,
                         (double2*)dst_vec);
    else
      hipLaunchKernelGGL(k_twin_transpose<false>, dim3(g), dim3(kBlock), 0, st, R, C, (const double*)src_vec,
                         (double*)dst_vec);
  } else {
    const DevIndex idx{src->d_off, src->d_rank, src->T.ns, src->T.nst - 1};
    const int nb = 2 * src->Mh.ns;
    const uint32_t full = nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
    if (vtype)
      hipLaunchKernelGGL(k_twin_gather<true>, dim3(grid_for(dim)), dim3(kBlock), 0, st, dst->d_map, dim, idx,
                         src->Mh.mode, full, (const double2*)src_vec, (double2*)dst_vec);
    else
      hipLaunchKernelGGL(k_twin_gather<false>, dim3(grid_for(dim)), dim3(kBlock), 0, st, dst->d_map, dim, idx,
                         src->Mh.mode, full, (const double*)src_vec, (double*)dst_vec);
  }
  HIPCK(hipGetLastError());
  return ED_OK;
}

// ------------------------------------------------ observables of a kept state
// (ed_obs.hpp).  Both calls make one grid-strided pass over (d_map, vec) on a
// grid of at most kObsMaxGrid blocks, then one finishing launch that sums
// every row of block partials in fixed order; the few results come back
// through a pinned block.  Nothing is kept in the sector object.
static constexpr int kObsMaxGrid = 1024;

// observables_impurity's diagonal loop (ED_OBSERVABLES.f90:127-158) and the
// density-density / Hartree sums of local_energy_impurity (:797-943) are
// linear in these moments.
int ed_sector_nn_moments(const ed_sector* s, int32_t vtype, const void* vec_dev, int32_t nlev,
                         const int32_t* levels, double* out, void* stream) {
  if (!s || !vec_dev || !levels || !out) return fail(ED_ERR_ARG, "null");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  static_assert(kObsMaxLev == 6, "launch_nn_moments instantiates 1..6 levels");
  if (nlev < 1 || nlev > kObsMaxLev) return fail(ED_ERR_ARG, "nlev must be 1..2*ED_MAX_NORB");
  ObsLevels L{};
  for (int p = 0; p < nlev; p++) {
    if (levels[p] < 0 || levels[p] >= 2 * s->Mh.ns) return fail(ED_ERR_ARG, "level outside the 2*Ns Fock levels");
    L.lev[p] = levels[p];
  }
  CK(whole_only(s));
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  const int nm = nlev * (nlev + 1) / 2 + 1;
  const int g = std::min(grid_for(s->dim), kObsMaxGrid);
  double* d = nullptr;
  HIPCK(hipMallocAsync((void**)&d, ((size_t)nm * g + nm) * sizeof(double), st));
  DevFree fr{d, st};
  PinnedLease pin((size_t)nm * sizeof(double), st);
  if (!pin.p) return fail(ED_ERR_OOM, "pinned staging");
  if (vtype) launch_nn_moments<true>(nlev, g, st, s->d_map, vec_dev, s->dim, L, d);
  else launch_nn_moments<false>(nlev, g, st, s->d_map, vec_dev, s->dim, L, d);
  HIPCK(hipGetLastError());
  hipLaunchKernelGGL(k_obs_finish, dim3(nm), dim3(kBlock), 0, st, d, g, d + (size_t)nm * g);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(pin.p, d + (size_t)nm * g, (size_t)nm * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  memcpy(out, pin.p, (size_t)nm * sizeof(double));
  return ED_OK;
}

// The off-diagonal sums of observables_impurity (ED_OBSERVABLES.f90:556-581,
// :631-654; magX/magY/phisc expanded, :166-337) and local_energy_impurity
// (:802-846 hopping, :882-927 spin exchange and pair hopping) as expectation
// values of operator strings.  Every string is compiled (and rejected if it
// leaves the sector) before anything is launched.
int ed_sector_expect(const ed_sector* s, int32_t vtype, const void* vec_dev, int32_t nterm, const int32_t* nops,
                     const int32_t* levels, const int32_t* ops, double* out, void* stream) {
  if (!s || !vec_dev || !nops || !levels || !ops || !out) return fail(ED_ERR_ARG, "null");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  if (nterm < 1) return fail(ED_ERR_ARG, "nterm must be positive");
  CK(whole_only(s));
  const ObsSector os{s->Mh.ns, s->Mh.mode, s->Mh.jz, s->Mh.lz2};
  const int ntp = (nterm + kObsTile - 1) / kObsTile * kObsTile;  // padded with null terms
  std::vector<ObsTerm> terms((size_t)ntp, obs_null_term());
  for (int t = 0, o = 0; t < nterm; t++) {
    if (nops[t] < 1 || nops[t] > kObsMaxOps)
      return fail(ED_ERR_ARG, "term " + std::to_string(t) + ": 1..4 operators per string");
    if (obs_compile(os, nops[t], levels + o, ops + o, &terms[t]) != ED_OK)
      return fail(ED_ERR_ARG, "term " + std::to_string(t) + ": bad level/op, or the string leaves the sector");
    o += nops[t];
  }
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  const int g = std::min(grid_for(s->dim), kObsMaxGrid);
  const int w = vtype ? 2 : 1;  // partial rows per term
  const size_t nval = (size_t)w * ntp;
  double* d = nullptr;
  HIPCK(hipMallocAsync((void**)&d, (nval * g + nval) * sizeof(double), st));
  DevFree fr{d, st};
  PinnedLease pin(nval * sizeof(double), st);
  if (!pin.p) return fail(ED_ERR_OOM, "pinned staging");
  const DevIndex idx{s->d_off, s->d_rank, s->T.ns, s->T.nst - 1};
  for (int t0 = 0; t0 < ntp; t0 += kObsMaxTerms) {
    const int n = std::min(kObsMaxTerms, ntp - t0);
    ObsTermList TL;
    for (int k = 0; k < kObsMaxTerms; k++) TL.t[k] = k < n ? terms[t0 + k] : obs_null_term();
    double* part = d + (size_t)w * t0 * g;
    if (vtype)
      hipLaunchKernelGGL(k_expect<true>, dim3(g), dim3(kBlock), 0, st, s->d_map, (const double2*)vec_dev, s->dim,
                         idx, TL, n, part);
    else
      hipLaunchKernelGGL(k_expect<false>, dim3(g), dim3(kBlock), 0, st, s->d_map, (const double*)vec_dev, s->dim,
                         idx, TL, n, part);
    HIPCK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_obs_finish, dim3((unsigned)nval), dim3(kBlock), 0, st, d, g, d + nval * g);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(pin.p, d + nval * g, nval * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  const double* h = (const double*)pin.p;
  for (int t = 0; t < nterm; t++) {
    out[2 * t] = vtype ? h[2 * t] : h[t];
    out[2 * t + 1] = vtype ? h[2 * t + 1] : 0.0;
  }
  return ED_OK;
}

}  // extern "C"
