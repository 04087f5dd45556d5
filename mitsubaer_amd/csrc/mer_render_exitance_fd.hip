// mer_render_exitance_fd.hip -- instantiations of the frequency-domain kind of K_exitance (mer_exitance.hpp, FD), in a translation unit of
// their own so that they compile beside the steady ones.  The launch and the entry points are mer_render_exitance.hip's.
#include "mer_lightpath_host.hpp"
#include "mer_exitance.hpp"

namespace mer {

struct ExitanceFDFamily {
    typedef void (*Kernel)(const Params, const ExitanceMap, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return exitance_kernel<CURVED, RIF, STEPPER, SIGMA, true>; }
};
ExitanceFDFamily::Kernel pick_exitance_fd(const mer_scene_desc *sc) { return pick_light_kernel<ExitanceFDFamily>(sc); }

}  // namespace mer
