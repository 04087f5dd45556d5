// mer_render_fluence_fd.hip -- instantiations of the frequency-domain kind of K_fluence (mer_fluence.hpp, FD), in a translation unit of their
// own so that they compile beside the steady and the time-resolved ones.  The launch and the entry points are mer_render_fluence.hip's.
#include "mer_lightpath_host.hpp"
#include "mer_fluence.hpp"

namespace mer {

struct FluenceFDFamily {
    typedef void (*Kernel)(const Params, const FluenceGrid, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return fluence_kernel<CURVED, RIF, STEPPER, SIGMA, false, true>; }
};
FluenceFDFamily::Kernel pick_fluence_fd(const mer_scene_desc *sc) { return pick_light_kernel<FluenceFDFamily>(sc); }

}  // namespace mer
