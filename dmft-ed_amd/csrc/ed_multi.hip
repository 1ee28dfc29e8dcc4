// ed_multi.hip — the launcher of the block stored H·X kernel (ed_multi.hpp),
// instantiated here once per block width and epilogue, and the entry point
// that applies H to a row-interleaved block of vectors.
#include "ed_sector.hpp"
#include "ed_multi.hpp"

using namespace edg;

// Blocks of a k_spmv_mv launch: the stored kernels' grid (hxv_blocks for the
// one-pass forms).  Every per-block reduction over the launch is sized by it.
int hxv_mv_blocks(const ed_sector* s) {
  const int g = grid_for(s->nslice * 64);
  return xcd_on(s, 0) ? (g & ~7) : g;
}

template <bool HC, bool VC, int NV, class Epi>
static int launch_hxv_mv_t(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  const int64_t dim = s->dim, ns = s->nslice;
  const int gx = hxv_mv_blocks(s);
  const int xr = xcd_on(s, 0) ? 1 : 0;
  // non-temporal matrix loads once the matrix cannot stay in the 256 MB MALL
  const bool nt = stored_mbytes(s) > ((int64_t)192 << 20);
#define ED_MV(NTV, PKV, CW, HV)                                                                               \
  hipLaunchKernelGGL((k_spmv_mv<HC, VC, NTV, NV, PKV, Epi>), dim3(gx), dim3(kBlock), 0, st, (const H*)s->d_diag, \
                     s->d_sptr, (const uint32_t*)(CW), (const H*)(HV), (const V*)x, dim, ns, epi, xr)
  if (s->d_words) {
    if (nt) ED_MV(1, true, s->d_words, s->d_pdict);
    else ED_MV(0, true, s->d_words, s->d_pdict);
  } else {
    if (nt) ED_MV(1, false, s->d_cols, s->d_vals);
    else ED_MV(0, false, s->d_cols, s->d_vals);
  }
#undef ED_MV
  HIPCK(hipGetLastError());
  return ED_OK;
}

template <bool VC, int NV, class Epi>
int launch_hxv_mv(ed_sector* s, const void* x, Epi epi, hipStream_t st) {
  if (s->hc) {
    if constexpr (VC) return launch_hxv_mv_t<true, true, NV>(s, x, epi, st);
    return fail(ED_ERR_ARG, "complex Hamiltonian needs complex vectors (vtype=1)");
  }
  return launch_hxv_mv_t<false, VC, NV>(s, x, epi, st);
}

#define ED_MV_INST(VC, NV)                                                                                  \
  template int launch_hxv_mv<VC, NV, EpiStoreMV<VC, NV>>(ed_sector*, const void*, EpiStoreMV<VC, NV>, hipStream_t); \
  template int launch_hxv_mv<VC, NV, EpiLancAMV<VC, NV>>(ed_sector*, const void*, EpiLancAMV<VC, NV>, hipStream_t);
ED_MV_INST(false, 1) ED_MV_INST(false, 2) ED_MV_INST(false, 4) ED_MV_INST(false, 8)
ED_MV_INST(true, 1) ED_MV_INST(true, 2) ED_MV_INST(true, 4) ED_MV_INST(true, 8)
#undef ED_MV_INST

// What the block kernel needs of a sector: the stored matrix, whole.
int mv_sector_check(const ed_sector* s) {
  if (!(s->flags & ED_STORED) || !s->d_sptr)
    return fail(ED_ERR_UNSUPPORTED, "sector has no stored matrix (the block H·X kernel reads the stored SELL form: ED_STORED)");
  if (s->nrows != s->dim)
    return fail(ED_ERR_UNSUPPORTED, "row-split sector: the block H·X kernel needs the whole stored matrix");
  return ED_OK;
}

extern "C" {

int ed_sector_hxv_multi(ed_sector* s, int32_t vtype, int32_t nvec, const void* x_dev, void* y_dev, void* stream) {
  // (what the arguments alone decide comes first: no sector is read for it)
  if (nvec != 1 && nvec != 2 && nvec != 4 && nvec != 8) return fail(ED_ERR_ARG, "nvec must be 1, 2, 4 or 8");
  if (vtype != 0 && vtype != 1) return fail(ED_ERR_ARG, "vtype must be 0 (real) or 1 (complex)");
  if (!x_dev || !y_dev) return fail(ED_ERR_ARG, "null block");
  if (x_dev == y_dev) return fail(ED_ERR_ARG, "y overlaps x (the kernel gathers x while rows of y are stored)");
  if (!s) return fail(ED_ERR_ARG, "null sector");
  if (vtype == 0 && s->hc) return fail(ED_ERR_ARG, "complex H needs vtype=1");
  const size_t bytes = (size_t)s->dim * nvec * (vtype ? 16 : 8);
  const uintptr_t a = (uintptr_t)x_dev, b = (uintptr_t)y_dev;
  if (a < b + bytes && b < a + bytes) return fail(ED_ERR_ARG, "y overlaps x (the kernel gathers x while rows of y are stored)");
  if ((a | b) & 15) return fail(ED_ERR_ARG, "x and y must be 16-byte aligned");
  CK(mv_sector_check(s));
  HIPCK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  return with_vc(vtype != 0, [&](auto c) -> int {
    constexpr bool VC = decltype(c)::value;
    using V = val_t<VC>;
    switch (nvec) {
      case 1: return launch_hxv_mv<VC, 1>(s, x_dev, EpiStoreMV<VC, 1>{(V*)y_dev}, st);
      case 2: return launch_hxv_mv<VC, 2>(s, x_dev, EpiStoreMV<VC, 2>{(V*)y_dev}, st);
      case 4: return launch_hxv_mv<VC, 4>(s, x_dev, EpiStoreMV<VC, 4>{(V*)y_dev}, st);
      default: return launch_hxv_mv<VC, 8>(s, x_dev, EpiStoreMV<VC, 8>{(V*)y_dev}, st);
    }
  });
}

}  // extern "C"
