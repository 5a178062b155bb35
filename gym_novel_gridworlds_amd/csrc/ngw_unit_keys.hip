// ngw_unit_keys.hip — state keys (ngw_keys.inc): 64-bit hashes of saved slots and live envs.
#include "ngw_common.inc"
#include "ngw_keys.inc"

// x->count keys of rows of x->src through the index list; one wave per 64 pairs
extern "C" hipError_t ngw_keys_launch(const NgwKeys* x, hipStream_t stream) {
    const int64_t blocks = blocks_for(x->count);
    if (x->count <= 0 || blocks > 0x7FFFFFFFll || x->rows < 1 || x->S2 < 9 || x->S2 > NGW_MAX_MAP_SIZE * NGW_MAX_MAP_SIZE || x->K < 1 || x->K > NGW_MAX_ITEMS ||
        !x->fields || (x->fields & ~NGW_KEY_ALL) || !x->flags || !x->src.map || !x->keys)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(NGW_EPB);
    return with_row_piece(x->S2, [&](auto V) { return launch_kernel<ngw_keys_kernel<decltype(V)::value>>(grid, block, 0, stream, *x); });
}
