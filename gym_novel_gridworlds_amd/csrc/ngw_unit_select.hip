// ngw_unit_select.hip — priority frontiers (ngw_select.inc): the `keep` best candidates of every group of values, as index lists of fixed capacity.
#include "ngw_common.inc"
#include "ngw_select.inc"

// the work-groups that fill `entries` list entries, four per thread, within what one call's grid may be
static unsigned select_fill_blocks(int64_t entries) {
    const int64_t blocks = (entries + 4 * NGW_FRONTIER_BLOCK - 1) / (4 * NGW_FRONTIER_BLOCK);
    return (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// The one place that decides which form runs: m <= NGW_SELECT_WAVE_MAX the wave form (one launch; the scratch's ticket word is 0 between the
// calls), above it the grid form (a memset of the scratch and six launches).
extern "C" hipError_t ngw_frontier_select_launch(const NgwSelect* x, hipStream_t stream) {
    const int64_t n = (int64_t)x->groups * x->m, tpg = ((int64_t)x->m + NGW_FRONTIER_TILE - 1) / NGW_FRONTIER_TILE;
    if (x->groups < 1 || x->groups > NGW_SELECT_MAX_VALUES || x->m < 0 || n > NGW_SELECT_MAX_VALUES || x->div < 1 || x->keep < 0 || x->capacity < 0 ||
        x->capacity > 0x7FFFFFFFll || (int64_t)x->groups * x->keep > x->capacity || (x->largest != 0 && x->largest != 1) ||
        (int64_t)x->tiles_per_group != tpg || (n && !x->values) || (x->capacity && !x->first) || !x->taken || !x->bound || !x->count || !x->scratch)
        return hipErrorInvalidValue;
    // what every thread fills in a grid stride: the lists' tail, and the entries from min(keep, m) on of every span
    const int64_t km = x->keep < x->m ? x->keep : x->m;
    const unsigned fill = select_fill_blocks(x->capacity - (int64_t)x->groups * km);
    const dim3 block(NGW_FRONTIER_BLOCK);
    if (x->m <= NGW_SELECT_WAVE_MAX) {
        int64_t work = ((int64_t)x->groups + 3) / 4;                               // a wave per group, up to 2048 work-groups
        if (work > 2048) work = 2048;
        const dim3 grid((unsigned)work > fill ? (unsigned)work : fill);
        return with_flag(x->m <= 4 * NGW_EPB, [&](auto SMALL) {
            return launch_kernel<ngw_select_wave_kernel<decltype(SMALL)::value ? 4 : 16>>(grid, block, 0, stream, *x, (int)work);
        });
    }
    const int64_t tiles = (int64_t)x->groups * tpg;
    hipError_t e = hipMemsetAsync(x->scratch, 0, (size_t)NGW_SELECT_SCRATCH_WORDS(x->groups, tpg) * sizeof(uint32_t), stream);
    const dim3 grid((unsigned)tiles);
    if (e == hipSuccess) e = launch_kernel<ngw_select_hist_kernel<0>>(grid, block, 0, stream, *x);
    if (e == hipSuccess) e = launch_kernel<ngw_select_hist_kernel<1>>(grid, block, 0, stream, *x);
    if (e == hipSuccess) e = launch_kernel<ngw_select_hist_kernel<2>>(grid, block, 0, stream, *x);
    if (e == hipSuccess) e = launch_kernel<ngw_select_hist_kernel<3>>(grid, block, 0, stream, *x);
    if (e == hipSuccess) e = launch_kernel<ngw_select_count_kernel>(grid, block, 0, stream, *x);
    if (e == hipSuccess) e = launch_kernel<ngw_select_scatter_kernel>(dim3((unsigned)tiles > fill ? (unsigned)tiles : fill), block, 0, stream, *x);
    return e;
}
