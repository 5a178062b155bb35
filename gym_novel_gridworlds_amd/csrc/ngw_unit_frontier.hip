// ngw_unit_frontier.hip — device-side frontiers (ngw_frontier.inc): flags compacted into index lists of fixed capacity, slots handed out for them.
#include "ngw_common.inc"
#include "ngw_frontier.inc"

// the work-groups that fill `capacity` entries, four per thread, within what one call's grid may be
static unsigned frontier_fill_blocks(int64_t capacity) {
    const int64_t blocks = (capacity + 4 * NGW_FRONTIER_BLOCK - 1) / (4 * NGW_FRONTIER_BLOCK);
    return (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// x->n flag bytes into x->first / x->second of x->capacity entries and x->count: the count launch over the tiles, then the scatter (n == 0: the
// scatter alone, which fills the lists with NGW_IDX_NONE and stores the two zeros)
extern "C" hipError_t ngw_frontier_compact_launch(const NgwFrontier* x, hipStream_t stream) {
    const int64_t tiles = (x->n + NGW_FRONTIER_TILE - 1) / NGW_FRONTIER_TILE;
    if (x->n < 0 || x->n > NGW_FRONTIER_MAX_FLAGS || x->capacity < 0 || x->capacity > 0x7FFFFFFFll || x->div < 1 || (int64_t)x->n_tiles != tiles ||
        (x->n && (!x->bytes || !x->tiles)) || (x->capacity && !x->first) || !x->count || !x->flags)
        return hipErrorInvalidValue;
    const unsigned fill = frontier_fill_blocks(x->capacity);
    const dim3 block(NGW_FRONTIER_BLOCK), count_grid((unsigned)tiles), scatter_grid((unsigned)tiles > fill ? (unsigned)tiles : fill);
    return with_flag((reinterpret_cast<uintptr_t>(x->bytes) & 15u) == 0, [&](auto V) {
        if (tiles) {
            const hipError_t e = launch_kernel<ngw_frontier_count_kernel<decltype(V)::value>>(count_grid, block, 0, stream, *x);
            if (e != hipSuccess) return e;
        }
        return launch_kernel<ngw_frontier_scatter_kernel<decltype(V)::value>>(scatter_grid, block, 0, stream, *x);
    });
}

// x->capacity slots from *x->cursor on, as many as x->count[0] asks for and x->limit leaves
extern "C" hipError_t ngw_frontier_alloc_launch(const NgwFrontierAlloc* x, hipStream_t stream) {
    if (x->capacity < 0 || x->capacity > 0x7FFFFFFFll || x->limit < 0 || !x->count || !x->cursor || !x->ticket || !x->flags || (x->capacity && !x->slots))
        return hipErrorInvalidValue;
    return launch_kernel<ngw_frontier_alloc_kernel>(dim3(frontier_fill_blocks(x->capacity)), dim3(NGW_FRONTIER_BLOCK), 0, stream, *x);
}
