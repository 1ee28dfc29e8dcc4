// ed_persist_launch.hpp — the k_lanc_persist launch templates (one-workgroup
// persistent Lanczos, ed_persist.hpp): dispatch on the sector's register-
// layout geometry down to one instantiation.  Shared by the three units that
// each instantiate one (HC, VC) case: ed_persist_launch.hip (complex H,
// complex v; and persist_launch itself), ed_persist_launch_rc.hip (real H,
// complex v) and ed_persist_launch_rr.hip (real H, real v).
#pragma once
#include <atomic>
#include <mutex>

#include "ed_host.hpp"
#include "ed_kernels.hpp"
#include "ed_persist.hpp"

namespace edg {

constexpr int kMaxDevices = 64;  // device ordinals with a remembered dynamic-LDS limit

template <bool HC, bool VC, int MODE, int RPT, int E = 1>
static int persist_launch_t(const PersistGeom& s, const PersistRun<HC>& run, int64_t lds, hipStream_t st, int nb) {
  if constexpr ((MODE == 2 || MODE == 3) && RPT * E > preg_cap(HC, VC)) {
    return fail(ED_ERR_UNSUPPORTED, "register-resident ELL exceeds the spill-free budget");
  } else if constexpr (MODE == 4 && (HC || (VC ? !pkr_fits_c512(E, RPT) : !pkr_fits(E, RPT)))) {
    return fail(ED_ERR_UNSUPPORTED, "Kronecker register layout: real H within the register budget");
  } else {
  constexpr int NT = MODE >= 2 ? kPRegBlock : kPBlock;
  auto fn = k_lanc_persist<HC, VC, MODE, RPT, E, NT>;
  // the dynamic-LDS limit of this instantiation on this device: raised when
  // a launch needs more than any before it, not set on every launch (host
  // threads raise it under the lock, so the last value set is the largest)
  static std::atomic<int64_t> lds_set[kMaxDevices];
  static std::mutex mu;
  const int dev = s.device;
  if (dev < 0 || dev >= kMaxDevices) {
    HIPCK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  } else if (lds > lds_set[dev].load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(mu);
    if (lds > lds_set[dev].load(std::memory_order_relaxed)) {
      HIPCK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      lds_set[dev].store(lds, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(fn, dim3(nb), dim3(NT), (size_t)lds, st, run);
  HIPCK(hipGetLastError());
  return ED_OK;
  }
}

template <bool HC, bool VC, int MODE, int W>
static int persist_launch_e(const PersistGeom& s, const PersistRun<HC>& run, int64_t lds, hipStream_t st, int nb) {
  switch (MODE == 2 ? s.preg_rpt : MODE == 3 ? s.kreg_rpt : s.pkr_rpt) {
    case 2: return persist_launch_t<HC, VC, MODE, 2, W>(s, run, lds, st, nb);
    case 4: return persist_launch_t<HC, VC, MODE, 4, W>(s, run, lds, st, nb);
    case 6: return persist_launch_t<HC, VC, MODE, 6, W>(s, run, lds, st, nb);
    case 8: return persist_launch_t<HC, VC, MODE, 8, W>(s, run, lds, st, nb);
    default: return persist_launch_t<HC, VC, MODE, 10, W>(s, run, lds, st, nb);
  }
}

template <bool HC, bool VC, int MODE>
static int persist_launch_m(const PersistGeom& s, const PersistRun<HC>& run, int64_t lds, hipStream_t st, int nb = 1) {
  if constexpr (MODE == 4) {
    if constexpr (HC) {
      return fail(ED_ERR_UNSUPPORTED, "MODE 4 needs a real H");
    } else {
      return s.pkr_E == 4 ? persist_launch_e<HC, VC, 4, 4>(s, run, lds, st, nb)
                           : persist_launch_e<HC, VC, 4, 8>(s, run, lds, st, nb);
    }
  } else if constexpr (MODE >= 2) {
    switch (MODE == 2 ? s.preg_E : s.kreg_W) {
      case 8: return persist_launch_e<HC, VC, MODE, 8>(s, run, lds, st, nb);
      case 12: return persist_launch_e<HC, VC, MODE, 12>(s, run, lds, st, nb);
      case 14: return persist_launch_e<HC, VC, MODE, 14>(s, run, lds, st, nb);
      default: return persist_launch_e<HC, VC, MODE, 16>(s, run, lds, st, nb);
    }
  } else {
  switch (persist_rpt01(s.dim)) {
    case 1: return persist_launch_t<HC, VC, MODE, 1>(s, run, lds, st, nb);
    case 2: return persist_launch_t<HC, VC, MODE, 2>(s, run, lds, st, nb);
    case 3: return persist_launch_t<HC, VC, MODE, 3>(s, run, lds, st, nb);
    case 4: return persist_launch_t<HC, VC, MODE, 4>(s, run, lds, st, nb);
    case 5: return persist_launch_t<HC, VC, MODE, 5>(s, run, lds, st, nb);
    case 6: return persist_launch_t<HC, VC, MODE, 6>(s, run, lds, st, nb);
    case 8: return persist_launch_t<HC, VC, MODE, 8>(s, run, lds, st, nb);
    case 10: return persist_launch_t<HC, VC, MODE, 10>(s, run, lds, st, nb);
    case 12: return persist_launch_t<HC, VC, MODE, 12>(s, run, lds, st, nb);
    default: return persist_launch_t<HC, VC, MODE, 16>(s, run, lds, st, nb);
  }
  }
}

template <bool HC, bool VC>
static int persist_launch_hv(int mode, const PersistGeom& g, const void* run, int64_t lds, hipStream_t st, int nb) {
  const PersistRun<HC>& r = *(const PersistRun<HC>*)run;
  switch (mode) {
    case 0: return persist_launch_m<HC, VC, 0>(g, r, lds, st, nb);
    case 1: return persist_launch_m<HC, VC, 1>(g, r, lds, st, nb);
    case 2: return persist_launch_m<HC, VC, 2>(g, r, lds, st, nb);
    case 3: return persist_launch_m<HC, VC, 3>(g, r, lds, st, nb);
    default: return persist_launch_m<HC, VC, 4>(g, r, lds, st, nb);
  }
}

}  // namespace edg
