// ngw_unit_step_wire.hip — the in-place step kernels with the host write-through and with the fused action masks, and the stand-alone mask
// kernel (ngw_mask.inc).
#include "ngw_common.inc"
#include "ngw_lean.inc"

// in-place step with the fused action masks
NGW_PART_FN(ngw_part_step_mask_ns) {
    return with_flag((feat & NGW_FEAT_EXT) != 0, [&](auto E) { return launch_lean<NGW_MAP_STRAIGHT, false, decltype(E)::value, false, 0, false, true>(dspec, a, grid, lds_bytes, stream); });
}

// in-place step with the host write-through (NgwWT: ngw_step_host_packed's steady state)
NGW_PART_FN(ngw_part_step_wire) {
    if (feat & NGW_FEAT_LIDAR) return ngw_part_step_wire_boards(dspec, a, feat, grid, lds_bytes, stream);
    return with_flag((feat & NGW_FEAT_EXT) != 0, [&](auto E) { return launch_lean<NGW_MAP_STRAIGHT, false, decltype(E)::value, false, 0, true>(dspec, a, grid, lds_bytes, stream); });
}

// the action masks of the state in HBM (ngw_mask.inc): [n_pad] uint64 words at `out`
extern "C" hipError_t ngw_mask_launch(const NgwDevSpec* dspec, const NgwBufs* b, int64_t n, int S, int K, int ext, uint64_t* out, unsigned grid, hipStream_t stream) {
    if (n <= 0 || n > 0xFFFFFFFFll || S < 3 || S > NGW_MAX_MAP_SIZE || K < 1 || K > NGW_MAX_ITEMS) return hipErrorInvalidValue;
    return with_flag(ext != 0, [&](auto E) { return launch_kernel<ngw_mask_kernel<decltype(E)::value>>(dim3(grid), dim3(NGW_EPB), 0, stream, dspec, *b, (uint32_t)n, S, K, out); });
}
