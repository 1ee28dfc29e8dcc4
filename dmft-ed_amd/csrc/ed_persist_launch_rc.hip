// ed_persist_launch_rc.hip — the k_lanc_persist instantiations for real H and
// complex vectors (called by persist_launch, ed_persist_launch.hip).
#include "ed_persist_launch.hpp"

namespace edg {

int persist_launch_rc(int mode, const PersistGeom& g, const void* run, int64_t lds, hipStream_t st, int nb) {
  return persist_launch_hv<false, true>(mode, g, run, lds, st, nb);
}

}  // namespace edg
