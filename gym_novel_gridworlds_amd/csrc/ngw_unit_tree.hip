// ngw_unit_tree.hip — tree-search runs (ngw_tree.inc): the leaf, grow, backup and reweight kernels between the guided playout and the table's insert of
// one MCTS iteration, and the reweight's 16-lane form (the spread rule).
#include "ngw_common.inc"
#include "ngw_tree.inc"

// the sizes every kernel checks its indices against, within what an int32 index holds
static bool tree_sizes_ok(const NgwTree* x) {
    return x->buckets >= 1 && x->buckets <= 0x7FFFFFFFll && x->A >= 1 && x->A <= NGW_MAX_ACTIONS && x->buckets * x->A <= 0x7FFFFFFFll && x->cap >= 1 &&
           x->cap <= 0x7FFFFFFFll && x->count >= 0 && x->count <= x->cap && x->T >= 1 && x->n >= 1 && x->n <= x->T && x->stride >= x->count &&
           (int64_t)x->T * x->cap <= 0x7FFFFFFFll && ((!x->row && !x->next_row) || (x->row && x->next_row && x->row != x->next_row));
}

static dim3 tree_grid(int64_t count) { return dim3((unsigned)((count + NGW_TREE_BLOCK - 1) / NGW_TREE_BLOCK)); }

extern "C" hipError_t ngw_tree_leaf_launch(const NgwTree* x, hipStream_t stream) {
    if (!tree_sizes_ok(x) || !x->depth || !x->length || !x->keys || !x->masks || !x->leaf_keys || !x->leaf_masks) return hipErrorInvalidValue;
    if (x->count == 0 && !x->row) return hipSuccess;
    return launch_kernel<ngw_tree_leaf_kernel>(tree_grid(x->count ? x->count : 1), dim3(NGW_TREE_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_tree_grow_launch(const NgwTree* x, hipStream_t stream) {
    if (!tree_sizes_ok(x) || !x->where_leaf || !x->leaf_keys || !x->leaf_masks || !x->fresh || !x->mask_words) return hipErrorInvalidValue;
    if (x->count == 0) return hipSuccess;
    return launch_kernel<ngw_tree_grow_kernel>(tree_grid(x->count), dim3(NGW_TREE_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_tree_backup_launch(const NgwTree* x, hipStream_t stream) {
    if (!tree_sizes_ok(x) || !x->visits || !x->returns || !x->touched || (x->count && (!x->depth || !x->length || !x->actions || !x->rewards || !x->where)))
        return hipErrorInvalidValue;
    return launch_kernel<ngw_tree_backup_kernel>(tree_grid(x->cap), dim3(NGW_TREE_BLOCK), 0, stream, *x);
}

// the backup under a discount g in [0, 65536) (65536 is the kernel above)
extern "C" hipError_t ngw_tree_backup_discount_launch(const NgwTree* x, const NgwTreeRule* r, hipStream_t stream) {
    if (!tree_sizes_ok(x) || r->g < 0 || r->g >= 65536 || !x->visits || !x->returns || !x->touched || (x->count && (!x->depth || !x->length || !x->actions || !x->rewards || !x->where)))
        return hipErrorInvalidValue;
    return launch_kernel<ngw_tree_backup_discount_kernel>(tree_grid(x->cap), dim3(NGW_TREE_BLOCK), 0, stream, *x, *r);
}

extern "C" hipError_t ngw_tree_reweight_launch(const NgwTree* x, hipStream_t stream) {
    if (x->buckets < 1 || x->buckets > 0x7FFFFFFFll || x->A < 1 || x->A > NGW_MAX_ACTIONS || x->buckets * x->A > 0x7FFFFFFFll || x->n_list < 0 ||
        x->n_list > 0x7FFFFFFFll || !x->visits || !x->returns || !x->mask_words || !x->rows || !x->flags || (x->n_list && !x->list))
        return hipErrorInvalidValue;
    if (x->n_list == 0) return hipSuccess;
    return launch_kernel<ngw_tree_reweight_kernel>(tree_grid(x->n_list), dim3(NGW_TREE_BLOCK), 0, stream, *x);
}

// one list entry per 16 lanes: 16 entries per work-group (n_list <= 2^31 - 1: at most 2^27 work-groups)
extern "C" hipError_t ngw_tree_reweight16_launch(const NgwTree* x, const NgwTreeRule* r, hipStream_t stream) {
    if (x->buckets < 1 || x->buckets > 0x7FFFFFFFll || x->A < 1 || x->A > NGW_MAX_ACTIONS || x->buckets * x->A > 0x7FFFFFFFll || x->n_list < 0 ||
        x->n_list > 0x7FFFFFFFll || r->spread < 1 || r->spread > 64 || !x->visits || !x->returns || !x->mask_words || !x->rows || !x->flags || (x->n_list && !x->list))
        return hipErrorInvalidValue;
    if (x->n_list == 0) return hipSuccess;
    return launch_kernel<ngw_tree_reweight16_kernel>(tree_grid(x->n_list * 16), dim3(NGW_TREE_BLOCK), 0, stream, *x, *r);
}
