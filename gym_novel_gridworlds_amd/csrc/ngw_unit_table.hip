// ngw_unit_table.hip — the key table (ngw_table.inc): a hash set of state keys, with a value and a tag per key where the table was created for them.
#include "ngw_common.inc"
#define NGW_TABLE_UNIT                                            // the kernels are this unit's; the walk (table_find) is everybody's
#include "ngw_table.inc"

// x->count keys offered to / looked up in the table of x->mask + 1 buckets; one lane per key
static bool table_args_ok(const NgwTable* x, bool insert) {
    const int64_t blocks = (x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK;
    return x->count > 0 && blocks <= 0x7FFFFFFFll && x->key && x->stamp && x->stored && x->flags && x->keys && x->where && (!insert || x->fresh) &&
           x->mask >= 1 && x->mask < 0x7FFFFFFFull && (x->mask & (x->mask + 1)) == 0;
}

static dim3 table_grid(int64_t count) { return dim3((unsigned)((count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK)); }

extern "C" hipError_t ngw_table_insert_launch(const NgwTable* x, hipStream_t stream) {
    if (!table_args_ok(x, true)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK)), block(NGW_TABLE_BLOCK);
    const hipError_t e = launch_kernel<ngw_table_probe_kernel<true>>(grid, block, 0, stream, *x);
    return e != hipSuccess ? e : launch_kernel<ngw_table_fresh_kernel<>>(grid, block, 0, stream, *x);
}

extern "C" hipError_t ngw_table_lookup_launch(const NgwTable* x, hipStream_t stream) {
    if (!table_args_ok(x, false)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((x->count + NGW_TABLE_BLOCK - 1) / NGW_TABLE_BLOCK)), block(NGW_TABLE_BLOCK);
    return launch_kernel<ngw_table_probe_kernel<false>>(grid, block, 0, stream, *x);
}

// the low halves of one call's words must not wrap: (uint32)base + count <= 2^32
extern "C" hipError_t ngw_table_insert_min_launch(const NgwTable* x, hipStream_t stream) {
    if (!table_args_ok(x, true) || !x->best || !x->tag || !x->values || !x->improved || (x->base & 0xFFFFFFFFull) + (uint64_t)x->count > (1ull << 32))
        return hipErrorInvalidValue;
    const dim3 grid = table_grid(x->count), block(NGW_TABLE_BLOCK);
    const hipError_t e = launch_kernel<ngw_table_probe_kernel<true, true>>(grid, block, 0, stream, *x);
    return e != hipSuccess ? e : launch_kernel<ngw_table_fresh_kernel<true>>(grid, block, 0, stream, *x);
}

extern "C" hipError_t ngw_table_renorm_launch(uint64_t* best, uint64_t buckets, hipStream_t stream) {
    if (!best || buckets < 2 || buckets > (1ull << 31)) return hipErrorInvalidValue;
    return launch_kernel<ngw_table_renorm_kernel>(table_grid((int64_t)buckets), dim3(NGW_TABLE_BLOCK), 0, stream, best, buckets);
}

static bool table_mask_ok(uint64_t mask) { return mask >= 1 && mask < 0x7FFFFFFFull && (mask & (mask + 1)) == 0; }

extern "C" hipError_t ngw_table_read_launch(const NgwTableRead* x, hipStream_t stream) {
    if (x->count <= 0 || x->count > 0x7FFFFFFFll * NGW_TABLE_BLOCK || !x->best || !x->tag || !x->flags || !x->where || !x->value || !x->tag_out ||
        !table_mask_ok(x->mask))
        return hipErrorInvalidValue;
    return launch_kernel<ngw_table_read_kernel>(table_grid(x->count), dim3(NGW_TABLE_BLOCK), 0, stream, *x);
}

extern "C" hipError_t ngw_table_trace_launch(const NgwTableTrace* x, hipStream_t stream) {
    if (x->count <= 0 || x->count > 0x7FFFFFFFll || !x->key || !x->tag || !x->flags || !x->where || !x->length || !x->root || x->T < 0 || (x->T > 0 && !x->plans) ||
        x->A < 1 || !table_mask_ok(x->mask) || (x->mask + 1) * (uint64_t)x->A > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    return launch_kernel<ngw_table_trace_kernel>(table_grid(x->count), dim3(NGW_TABLE_BLOCK), 0, stream, *x);
}
