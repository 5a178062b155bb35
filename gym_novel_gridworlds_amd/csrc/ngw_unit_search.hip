// ngw_unit_search.hip — search runs (ngw_search.inc): the offer, judge and settle kernels between the five stages of a best-first iteration, and the roots;
// for an open-list search the take and open kernels, and the settle and roots kernels with the open-list work.
#include "ngw_common.inc"
#include "ngw_search.inc"

// capacity * A positions, each within what one insert_min / compaction takes, and every array the three kernels share
static bool search_args_ok(const NgwSearch* x) {
    return x->capacity >= 1 && x->capacity <= 0x7FFFFFFFll && x->pool >= 1 && x->pool <= 0x7FFFFFFFll && x->A >= 1 && x->A <= NGW_MAX_ACTIONS &&
           x->capacity * x->A <= NGW_FRONTIER_MAX_FLAGS && x->parents && x->next && x->g && x->bucket && x->info && x->lut && x->values && x->tags &&
           x->where && x->best && x->first && x->second && x->slots && x->plist && x->goal && x->overflowed && x->row && x->next_row &&
           x->row != x->next_row;
}

// an open-list search: every array of it, the bucket count and the heuristic's arguments together or not at all
static bool search_is_open(const NgwSearch* x) { return x->f != nullptr; }

static bool search_open_args_ok(const NgwSearch* x) {
    return search_args_ok(x) && x->f && x->h && x->slot_of_bucket && x->sel_count && x->orow && x->next_orow && x->orow != x->next_orow && x->buckets >= 1 &&
           x->buckets <= 0x7FFFFFFFll && (x->dist ? x->weights && x->K >= 1 && (x->mode == NGW_SEARCH_H_MIN || x->mode == NGW_SEARCH_H_MAX) : true);
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
    if (search_is_open(x)) {
        if (!search_open_args_ok(x)) return hipErrorInvalidValue;
        return launch_kernel<ngw_search_settle_kernel<true>>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
    }
    if (!search_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_settle_kernel<false>>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_take_launch(const NgwSearch* x, hipStream_t stream) {
    if (!search_open_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_take_kernel>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_open_launch(const NgwSearch* x, hipStream_t stream) {
    if (!search_open_args_ok(x)) return hipErrorInvalidValue;
    return launch_kernel<ngw_search_open_kernel>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_search_roots_launch(const NgwSearchRoots* x, hipStream_t stream) {
    if (x->capacity < 1 || x->capacity > 0x7FFFFFFFll || x->count < 0 || x->count > x->capacity || x->pool < 1 || x->pool > 0x7FFFFFFFll || !x->parents || !x->g ||
        !x->bucket || (x->count && (!x->roots || !x->where || !x->value || !x->best)))
        return hipErrorInvalidValue;
    if (x->f) {
        if (!x->h || !x->slot_of_bucket || x->buckets < 1 || x->buckets > 0x7FFFFFFFll ||
            (x->dist && (!x->weights || x->K < 1 || (x->mode != NGW_SEARCH_H_MIN && x->mode != NGW_SEARCH_H_MAX))))
            return hipErrorInvalidValue;
        return launch_kernel<ngw_search_roots_kernel<true>>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
    }
    return launch_kernel<ngw_search_roots_kernel<false>>(search_grid(x->capacity), dim3(NGW_SEARCH_BLOCK), 0, stream, *x);
}
