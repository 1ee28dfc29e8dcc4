// ed_persist_launch.hip — persist_launch, and the k_lanc_persist
// instantiations for complex H (complex vectors).  The real-H cases are two
// units of their own (ed_persist_launch_rc.hip, ed_persist_launch_rr.hip):
// the ~150 instantiations are half of the library's device compile, and the
// three cases compile in parallel.
#include "ed_persist_launch.hpp"

namespace edg {

// real H: complex vectors (ed_persist_launch_rc.hip), real vectors (ed_persist_launch_rr.hip)
int persist_launch_rc(int mode, const PersistGeom& g, const void* run, int64_t lds, hipStream_t st, int nb);
int persist_launch_rr(int mode, const PersistGeom& g, const void* run, int64_t lds, hipStream_t st, int nb);

int persist_launch(bool hc, bool vc, int mode, const PersistGeom& g, const void* run, int64_t lds,
                   hipStream_t st, int nb) {
  if (hc) {
    if (!vc) return fail(ED_ERR_ARG, "complex H needs complex vectors");
    if (mode == 4) return fail(ED_ERR_UNSUPPORTED, "MODE 4 needs real H");
    return persist_launch_hv<true, true>(mode, g, run, lds, st, nb);
  }
  return vc ? persist_launch_rc(mode, g, run, lds, st, nb)
            : persist_launch_rr(mode, g, run, lds, st, nb);
}

}  // namespace edg
