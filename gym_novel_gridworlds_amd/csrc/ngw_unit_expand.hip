// ngw_unit_expand.hip — snapshot expand (ngw_expand.inc).
#include "ngw_common.inc"
#include "ngw_expand.inc"

// a = the handle's rollout layout with a.autoreset, a.horizon; one wave per 64 pairs
extern "C" hipError_t ngw_expand_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwExpand* x, int ext, size_t lds_bytes, hipStream_t stream) {
    if (x->count <= 0 || x->src_rows < 1 || x->dst_rows < 1 || a->S < 3 || a->S > NGW_MAX_MAP_SIZE || a->K < 1 || a->K > NGW_MAX_ITEMS || a->MS < a->S2 ||
        (a->MS & 3) || !a->b.flags || !x->actions || !x->src.map || !x->dst.map)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks_for(x->count)), block(NGW_EPB);
    return with_row_piece(a->S2, [&](auto V) {
        return with_flag(ext != 0, [&](auto E) {
            return launch_kernel<ngw_expand_kernel<decltype(V)::value, decltype(E)::value>>(grid, block, lds_bytes, stream, dspec, *a, *x);
        });
    });
}
