// mer_render_fluence_track.hip -- instantiations of K_fluence_track (mer_fluence_track.hpp), the track-length estimator of the fluence grid:
// the 14 combinations pick_fluence (mer_render_fluence.hip) selects from.  The host loop and the entry points are mer_render_fluence.hip's.
#include "mer_internal.hpp"
#include "mer_fluence_track.hpp"

namespace mer {

typedef void (*FluenceKernel)(const Params, const FluenceGrid, uint64_t, uint32_t);

template <bool CURVED, int RIF, int STEPPER> static FluenceKernel pick_sigma(int sigma) {
    return sigma == MER_SIGMA_GRID ? fluence_track_kernel<CURVED, RIF, STEPPER, MER_SIGMA_GRID> : fluence_track_kernel<CURVED, RIF, STEPPER, MER_SIGMA_HOMOGENEOUS>;
}
template <int RIF> static FluenceKernel pick_curved(int stepper, int sigma) {
    if (stepper == MER_STEP_VERLET) return pick_sigma<true, RIF, MER_STEP_VERLET>(sigma);
    if (stepper == MER_STEP_RK4) return pick_sigma<true, RIF, MER_STEP_RK4>(sigma);
    return nullptr;
}
FluenceKernel pick_fluence_track(const mer_scene_desc *sc) {
    const int sigma = sc->sigma_mode == MER_SIGMA_GRID ? MER_SIGMA_GRID : MER_SIGMA_HOMOGENEOUS;
    switch (sc->rif_mode) {
    case MER_RIF_CONST: return pick_sigma<false, MER_RIF_TRILINEAR, MER_STEP_VERLET>(sigma);
    case MER_RIF_TRILINEAR: return pick_curved<MER_RIF_TRILINEAR>(sc->stepper, sigma);
    case MER_RIF_BSPLINE3: return pick_curved<MER_RIF_BSPLINE3>(sc->stepper, sigma);
    case MER_RIF_ACOUSTIC: return pick_curved<RIFK_ACOUSTIC>(sc->stepper, sigma);
    }
    return nullptr;
}

}  // namespace mer
