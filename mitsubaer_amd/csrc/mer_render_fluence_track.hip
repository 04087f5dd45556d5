// mer_render_fluence_track.hip -- instantiations of K_fluence_track (mer_fluence_track.hpp), the track-length estimator of the fluence grid,
// in a translation unit of their own so that they compile beside K_fluence's.  The launch and the entry points are mer_render_fluence.hip's.
#include "mer_lightpath_host.hpp"
#include "mer_fluence_track.hpp"

namespace mer {

struct FluenceTrackFamily {
    typedef void (*Kernel)(const Params, const FluenceGrid, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return fluence_track_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};
FluenceTrackFamily::Kernel pick_fluence_track(const mer_scene_desc *sc) { return pick_light_kernel<FluenceTrackFamily>(sc); }

}  // namespace mer
