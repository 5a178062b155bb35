// ngw_unit_step_boards.hip — the bit-row (boards) lidar: the in-place step kernels with the O(1) observation, ngw_boards_kernel and
// ngw_lidar_boards_kernel (ngw_boards.inc).
#include "ngw_common.inc"
#include "ngw_boards.inc"
#include "ngw_lean.inc"

NGW_PART_FN(ngw_part_step_boards) { return step_boards<false>(dspec, a, feat, grid, lds_bytes, stream); }

// bit rows of `rows` (a multiple of 64) maps at `map` -> `brd`; a = the launch's own LDS layout (maps at off_map, word tile at off_ltile, magicK = ceil(2^32 / BS))
extern "C" hipError_t ngw_boards_launch(const NgwLaunch* a, int map_mode, const int8_t* map, uint32_t* brd, int64_t rows, size_t lds_bytes, hipStream_t stream) {
    return with_map_mode(map_mode, [&](auto MM) {
        return launch_kernel<ngw_boards_kernel<decltype(MM)::value>>(dim3((unsigned)(rows / NGW_EPB)), dim3(NGW_EPB), lds_bytes, stream, *a, map, brd);
    });
}

extern "C" hipError_t ngw_lidar_boards_launch(const NgwLaunch* a, unsigned grid, size_t lds_bytes, hipStream_t stream) {
    return with_board_rows(a->BS, [&](auto R) { return launch_kernel<ngw_lidar_boards_kernel<decltype(R)::value>>(dim3(grid), dim3(NGW_EPB), lds_bytes, stream, *a); });
}
