// ngw_unit_step_straight.hip — the staged step kernels of the straight map mode, the plain in-place step kernels, and ngw_part_step, which
// sends a batched step() to the unit that holds its kernel.
#include "ngw_common.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_step_straight) { return step_staged<NGW_MAP_STRAIGHT>(dspec, a, feat, grid, lds_bytes, stream); }

extern "C" hipError_t ngw_part_step(const NgwDevSpec* dspec, const NgwLaunch* a, int map_mode, int feat, unsigned grid, size_t lds_bytes,
                                    hipStream_t stream) {
    if (feat & NGW_FEAT_NOSTAGE) {   // no-stage: with the lidar observation, the one on the occupancy bit rows
        if (feat & NGW_FEAT_WIRE) return ngw_part_step_wire(dspec, a, feat, grid, lds_bytes, stream);   // ... with the host write-through
        if (feat & NGW_FEAT_LIDAR) return ngw_part_step_boards(dspec, a, feat, grid, lds_bytes, stream);
        if (feat & NGW_FEAT_MASK) return ngw_part_step_mask_ns(dspec, a, feat, grid, lds_bytes, stream);
        if (feat & NGW_FEAT_VIEW) return ngw_part_step_view(dspec, a, feat, grid, lds_bytes, stream);   // ... with the fused AgentMap window
        if (feat & NGW_FEAT_EXT) return launch_lean<NGW_MAP_STRAIGHT, false, true, false>(dspec, a, grid, lds_bytes, stream);
        // ... the plain spec class has an instantiation of its own (launch_lean takes the launch back to the general one if it does not fit)
        return with_flag((feat & NGW_FEAT_PLAIN) != 0, [&](auto P) { return launch_lean<NGW_MAP_STRAIGHT, false, false, false, 0, false, false, decltype(P)::value>(dspec, a, grid, lds_bytes, stream); });
    }
    switch (map_mode) {
    case NGW_MAP_STRAIGHT: return ngw_part_step_straight(dspec, a, feat, grid, lds_bytes, stream);
    case NGW_MAP_DWORD: return ngw_part_step_dword(dspec, a, feat, grid, lds_bytes, stream);
    default: return ngw_part_step_byte(dspec, a, feat, grid, lds_bytes, stream);
    }
}
