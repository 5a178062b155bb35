// ngw_unit_step_view.hip — the in-place step kernels with the fused AgentMap window (ngw_step_lean<..., VIEW>, ngw_lean_step.inc): the plain spec
// class (and the general instantiation its launcher falls back to) and the one with the wrapper predicates.  No lidar, no masks, no host write-through.
#include "ngw_common.inc"
#include "ngw_lean.inc"

// `a` points at an NgwLaunchView (NGW_FEAT_VIEW)
NGW_PART_FN(ngw_part_step_view) {
    if (feat & NGW_FEAT_EXT) return launch_lean<NGW_MAP_STRAIGHT, false, true, false, 0, false, false, false, true>(dspec, a, grid, lds_bytes, stream);
    return with_flag((feat & NGW_FEAT_PLAIN) != 0, [&](auto P) { return launch_lean<NGW_MAP_STRAIGHT, false, false, false, 0, false, false, decltype(P)::value, true>(dspec, a, grid, lds_bytes, stream); });
}
