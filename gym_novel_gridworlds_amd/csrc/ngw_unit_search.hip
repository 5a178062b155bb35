// ngw_unit_search.hip — search runs (ngw_search.inc): the offer, judge and settle kernels between the five stages of a best-first iteration, and the roots.
#include "ngw_common.inc"
#include "ngw_search.inc"

// capacity * A positions, each within what one insert_min / compaction takes, and every array the three kernels share
static bool search_args_ok(const NgwSearch* x) {
    return x->capacity >= 1 && x->capacity <= 0x7FFFFFFFll && x->pool >= 1 && x->pool <= 0x7FFFFFFFll && x->A >= 1 && x->A <= NGW_MAX_ACTIONS &&
           x->capacity * x->A <= NGW_FRONTIER_MAX_FLAGS && x->parents && x->next && x->g && x->bucket && x->info && x->lut && x->values && x->tags &&
           x->where && x->best && x->first && x->second && x->slots && x->plist && x->goal && x->overflowed && x->row && x->next_row &&
           x->row != x->next_row;
}

static dim3 search_grid(int64_t count) { return dim3((unsigned)((count + NGW_SEARCH_BLOCK - 1) / NGW_SEARCH_BLOCK)); }

extern "C" hipError_t ngw_search_offer_launch(const NgwSearch* x, hipStream_t stream) {
    if (!search_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_offer_kernel>(search_grid(x->capacity * x->A), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_judge_launch(const NgwSearch* x, hipStream_t stream) {
    if (!search_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_judge_kernel>(search_grid(x->capacity * x->A), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_settle_launch(const NgwSearch* x, hipStream_t stream) {
    if (!search_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_settle_kernel>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_roots_launch(const NgwSearchRoots* x, hipStream_t stream) {
    if (x->capacity < 1 || x->capacity > 0x7FFFFFFFll || x->count < 0 || x->count > x->capacity || x->pool < 1 || x->pool > 0x7FFFFFFFll || !x->parents || !x->g ||
        !x->bucket || (x->count && (!x->roots || !x->where || !x->value || !x->best)))
        return hipErrorInvalidValue;
    return launch_kernel<ngw_search_roots_kernel>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}
