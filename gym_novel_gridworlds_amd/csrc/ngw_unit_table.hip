// ngw_unit_table.hip — the key table (ngw_table.inc): a hash set of state keys.
#include "ngw_common.inc"
#define NGW_TABLE_UNIT                                            // the three kernels are this unit's; the walk (table_find) is everybody's
#include "ngw_table.inc"

// x->count keys offered to / looked up in the table of x->mask + 1 buckets; one lane per key
static bool table_args_ok(const NgwTable* x, bool insert) {
    const int64_t blocks = (x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK;
    return x->count > 0 && blocks <= 0x7FFFFFFFll && x->key && x->stamp && x->stored && x->flags && x->keys && x->where && (!insert || x->fresh) &&
           x->mask >= 1 && x->mask < 0x7FFFFFFFull && (x->mask & (x->mask + 1)) == 0;
}

extern "C" hipError_t ngw_table_insert_launch(const NgwTable* x, hipStream_t stream) {
    if (!table_args_ok(x, true)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK)), block(NGW_TABLE_BLOCK);
    const hipError_t e = launch_kernel<ngw_table_probe_kernel<true>>(grid, block, 0, stream, *x);
    return e != hipSuccess ? e : launch_kernel<ngw_table_fresh_kernel>(grid, block, 0, stream, *x);
}

extern "C" hipError_t ngw_table_lookup_launch(const NgwTable* x, hipStream_t stream) {
    if (!table_args_ok(x, false)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK)), block(NGW_TABLE_BLOCK);
    return launch_kernel<ngw_table_probe_kernel<false>>(grid, block, 0, stream, *x);
}
