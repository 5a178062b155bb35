// ngw_unit_walk.hip — walk distances and go-to plans (ngw_walk.inc): shortest paths over (row, column, facing) of saved slots and live envs.
#include "ngw_common.inc"
#include "ngw_walk.inc"

// x->count rows of x->src through the index list; one wave per row, 32-bit row words up to 32 x 32 and 64-bit ones above, the walk back only
// where plans are asked for
extern "C" hipError_t ngw_walk_launch(const NgwWalk* x, hipStream_t stream) {
    const bool plans = x->items != nullptr;
    if (x->count <= 0 || x->count > 0x7FFFFFFFll || x->rows < 1 || x->S < 3 || x->S > NGW_MAX_MAP_SIZE || x->K < 1 || x->K > NGW_MAX_ITEMS ||
        x->SP != NGW_WALK_SP(x->S) || !x->flags || !x->src.map || !x->src.loc || !x->src.facing || (!x->dist && !(plans && (x->plans || x->length))) ||
        (plans && x->T < 1))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)x->count), block(NGW_EPB);
    const size_t lds_bytes = NGW_WALK_LDS_BYTES(x->S);
    return with_flag(x->S > 32, [&](auto WIDE) {
        using W = std::conditional_t<decltype(WIDE)::value, uint64_t, uint32_t>;
        return with_flag(plans, [&](auto P) { return launch_kernel<ngw_walk_kernel<W, decltype(P)::value>>(grid, block, lds_bytes, stream, *x); });
    });
}
