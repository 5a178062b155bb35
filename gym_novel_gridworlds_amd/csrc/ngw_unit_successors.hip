// ngw_unit_successors.hip — successor keys (ngw_successors.inc): the key of every action's child.
#include "ngw_common.inc"
#include "ngw_successors.inc"

// a = the handle's launch block with a.autoreset, a.horizon (S, K, MS, KP and the flags word are read; the kernel carves its own LDS:
// NGW_SUCC_LDS_BYTES); one wave per 64 parents
extern "C" hipError_t ngw_successors_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwSuccessors* x, int ext, hipStream_t stream) {
    const int64_t blocks = blocks_for(x->count);
    if (x->count <= 0 || blocks > 0x7FFFFFFFll || x->rows < 1 || a->S < 3 || a->S > NGW_MAX_MAP_SIZE || a->K < 1 || a->K > NGW_MAX_ITEMS || a->MS < a->S2 ||
        (a->MS & 3) || a->KP < a->K || NGW_SUCC_LDS_BYTES(a->MS, a->KP) > NGW_SUCC_LDS_MAX || !x->fields || (x->fields & ~NGW_KEY_ALL) || !a->b.flags ||
        !x->src.map || !x->keys)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(NGW_EPB);
    return with_row_piece(a->S2, [&](auto V) {
        return with_flag(ext != 0, [&](auto E) {
            return launch_kernel<ngw_successors_kernel<decltype(V)::value, decltype(E)::value>>(grid, block, NGW_SUCC_LDS_BYTES(a->MS, a->KP), stream, dspec, *a, *x);
        });
    });
}
