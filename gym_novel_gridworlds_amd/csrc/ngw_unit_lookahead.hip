// ngw_unit_lookahead.hip — one-step lookahead tables (ngw_lookahead.inc).
#include "ngw_common.inc"
#include "ngw_lookahead.inc"

// the one-step lookahead table of the state in HBM: action-major [n_actions][n_pad] reward / done / info
extern "C" hipError_t ngw_lookahead_launch(const NgwDevSpec* dspec, const NgwBufs* b, int64_t n, int64_t n_pad, int S, int K, int ext, int autoreset, int horizon,
                                           int32_t* reward, uint8_t* done, uint32_t* info, unsigned grid, hipStream_t stream) {
    if (n <= 0 || n > 0xFFFFFFFFll || n_pad < n || (int64_t)grid * NGW_EPB != n_pad || S < 3 || S > NGW_MAX_MAP_SIZE || K < 1 || K > NGW_MAX_ITEMS ||
        !reward || !done || !info)
        return hipErrorInvalidValue;
    return with_flag(ext != 0, [&](auto E) {
        return launch_kernel<ngw_lookahead_kernel<decltype(E)::value>>(dim3(grid), dim3(NGW_EPB), 0, stream, dspec, *b, (uint32_t)n, S, K, autoreset, horizon, (uint64_t)n_pad, reward, done, info);
    });
}
