// ngw_unit_sample.hip — the weighted choice among valid actions, one per state (ngw_sample.inc).
#include "ngw_common.inc"
#include "ngw_sample.inc"

// x->count pairs of rows of x->src through the index list; one wave per 64 pairs, no dynamic LDS
extern "C" hipError_t ngw_sample_launch(const NgwDevSpec* dspec, const NgwSample* x, int S, int K, int ext, hipStream_t stream) {
    if (x->count <= 0 || x->rows < 1 || x->stride < x->count || S < 3 || S > NGW_MAX_MAP_SIZE || K < 1 || K > NGW_MAX_ITEMS || !x->flags || !x->src.map ||
        !x->weights || !x->actions)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    return with_flag(ext != 0, [&](auto E) { return launch_kernel<ngw_sample_kernel<decltype(E)::value>>(grid, block, 0, stream, dspec, *x, S, K); });
}
