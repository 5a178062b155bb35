// ngw_abi_table.cpp - device-side key tables (see ngw_host.h): an open-addressing hash set of 64-bit keys per table, in one allocation of the
// handle, and the kernels (ngw_table.inc) that offer keys to it and look them up; a valued table keeps the smallest value offered with each key
// and a tag beside it (insert_min, read, trace).  The calls write no env state: they neither call
// state_written() nor touch anything the handle derives from its state.  Every entry point runs on the handle's stream, behind enter(): a
// table is only ever used in the order of the calls on that one stream (concurrent inserts from two streams are not supported).
#include "ngw_host.h"

using namespace ngwh;

namespace {

// the two arrays of a valued table, behind the counter
uint64_t* best_of(const ngw_key_table* t) { return t->slab + 2 * t->buckets + 1; }
int32_t* tag_of(const ngw_key_table* t) { return reinterpret_cast<int32_t*>(t->slab + 3 * t->buckets + 1); }

// best[] all ones (never valued) and tag[] all ones (-1 = NGW_TAG_ROOT): buckets + buckets / 2 words in one fill
hipError_t wipe_values(ngw_handle* h, ngw_key_table* t) {
    return hipMemsetAsync(best_of(t), 0xFF, (size_t)(t->buckets + t->buckets / 2) * 8, h->stream);
}

// key[] zero-filled, stamp[] all ones, the counter 0: the table as it is created, on the handle's stream
int wipe(ngw_handle* h, ngw_key_table* t) {
    const size_t words = (size_t)t->buckets;
    HIP_TRY(hipMemsetAsync(t->slab, 0, words * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->slab + words, 0xFF, words * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->slab + 2 * words, 0, 8, h->stream));
    if (t->valued) HIP_TRY(wipe_values(h, t));
    t->base = t->first;
    t->epoch = t->first >> 32;
    return NGW_OK;
}

NgwTable table_args(const ngw_handle* h, const ngw_key_table* t, const uint64_t* keys_dev, int64_t count, int32_t* where_dev, uint8_t* fresh_dev) {
    NgwTable x{};
    x.key = t->slab; x.stamp = t->slab + t->buckets; x.stored = reinterpret_cast<unsigned long long*>(t->slab + 2 * t->buckets);
    x.flags = h->b.flags; x.keys = keys_dev; x.where = where_dev; x.fresh = fresh_dev;
    x.base = t->base; x.mask = t->buckets - 1; x.count = count;
    return x;
}

// what insert and lookup check alike (before anything touches the stream)
int table_call_args(const ngw_handle* h, const ngw_key_table* t, const void* keys_dev, const void* out_a, const void* out_b, int64_t count) {
    if (!h || !t || !keys_dev || !out_a || !out_b) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->tables, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (count < 0 || count > 0x7FFFFFFFll * NGW_TABLE_BLOCK) return fail(NGW_E_INVALID_ARG, "key table call with %lld keys", (long long)count);
    return NGW_OK;
}

// a table with or without values: key[] | stamp[] | the counter, and for values best[] | tag[] (half as many words) behind them
int create_table(ngw_handle* h, int64_t capacity, bool valued, uint64_t first_sequence, ngw_key_table** out) {
    if (!h || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (capacity < 1 || capacity > (1ll << 29)) return fail(NGW_E_INVALID_ARG, "key table capacity %lld outside [1, 2^29]", (long long)capacity);
    if (first_sequence > (1ull << 62)) return fail(NGW_E_INVALID_ARG, "key table first_sequence %llu beyond 2^62", (unsigned long long)first_sequence);
    if (int rc = enter(h)) return rc;
    uint64_t buckets = 2;
    while (buckets < 2 * (uint64_t)capacity) buckets <<= 1;
    uint64_t* slab = nullptr;
    if (int rc = dev_alloc(h, &slab, (size_t)(2 * buckets + 1 + (valued ? buckets + buckets / 2 : 0)))) return rc;      // (zero-filled on the handle's stream)
    ngw_key_table* t = new ngw_key_table;
    t->cap = capacity; t->buckets = buckets; t->slab = slab; t->valued = valued; t->first = t->base = first_sequence; t->epoch = first_sequence >> 32;
    hipError_t e = hipMemsetAsync(slab + buckets, 0xFF, (size_t)buckets * 8, h->stream);
    if (e == hipSuccess && valued) e = wipe_values(h, t);
    if (e != hipSuccess) {
        dev_free(h, slab);
        delete t;
        return fail(NGW_E_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    h->tables.push_back(t);
    *out = t;
    return NGW_OK;
}

// what read and trace check alike: an open valued table of the handle, a bucket list and its outputs
int valued_call_args(const ngw_handle* h, const ngw_key_table* t, const void* where_dev, const void* out_a, const void* out_b, int64_t count, int64_t most) {
    if (!h || !t || !where_dev || !out_a || !out_b) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->tables, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (!t->valued) return fail(NGW_E_INVALID_ARG, "a key table without values (ngw_key_table_create_valued makes one with)");
    if (count < 0 || count > most) return fail(NGW_E_INVALID_ARG, "key table call with %lld buckets", (long long)count);
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_key_table_create(ngw_handle* h, int64_t capacity, ngw_key_table** out) { return create_table(h, capacity, false, 0, out); }

int ngw_key_table_create_valued(ngw_handle* h, int64_t capacity, uint64_t first_sequence, ngw_key_table** out) {
    return create_table(h, capacity, true, first_sequence, out);
}

int ngw_key_table_destroy(ngw_handle* h, ngw_key_table* t) {
    if (!h || !t) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->tables, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                         // (queued inserts / lookups may still use the table)
    for (size_t i = 0; i < h->tables.size(); i++)
        if (h->tables[i] == t) { h->tables.erase(h->tables.begin() + (long)i); break; }
    dev_free(h, t->slab);
    delete t;
    return NGW_OK;
}

int ngw_key_table_clear(ngw_handle* h, ngw_key_table* t) {
    if (!h || !t) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->tables, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (int rc = enter(h)) return rc;
    return wipe(h, t);
}

int ngw_key_table_insert(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, int64_t count, int32_t* where_dev, uint8_t* fresh_dev) {
    if (int rc = table_call_args(h, t, keys_dev, where_dev, fresh_dev, count)) return rc;
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    const NgwTable x = table_args(h, t, keys_dev, count, where_dev, fresh_dev);
    HIP_TRY(ngw_table_insert_launch(&x, h->stream));
    t->base += (uint64_t)count;                                       // (stamps only grow from call to call)
    return NGW_OK;
}

int ngw_key_table_insert_min(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, const int32_t* values_dev, const int32_t* tags_dev, int64_t count,
                             int32_t* where_dev, uint8_t* fresh_dev, uint8_t* best_dev) {
    if (int rc = table_call_args(h, t, keys_dev, where_dev, fresh_dev, count)) return rc;
    if (!values_dev || !best_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!t->valued) return fail(NGW_E_INVALID_ARG, "a key table without values (ngw_key_table_create_valued makes one with)");
    if (count > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "ngw_key_table_insert_min with %lld keys (at most 2^31 - 1)", (long long)count);
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    // The words in the table carry low halves of positions whose high half was t->epoch.  Where this call's positions have another high half - plain
    // inserts have carried base past a multiple of 2^32 -, or would pass one inside the call, the low halves would no longer grow: start them again above 0.
    if ((t->base >> 32) != t->epoch || (t->base & 0xFFFFFFFFull) + (uint64_t)count > (1ull << 32)) {
        HIP_TRY(ngw_table_renorm_launch(best_of(t), t->buckets, h->stream));
        t->base = (((t->base >> 32) + 1) << 32) | 1;                  // (the stamps only ask that base grows)
        t->epoch = t->base >> 32;
    }
    NgwTable x = table_args(h, t, keys_dev, count, where_dev, fresh_dev);
    x.best = best_of(t); x.tag = tag_of(t); x.values = values_dev; x.tags = tags_dev; x.improved = best_dev;
    HIP_TRY(ngw_table_insert_min_launch(&x, h->stream));
    t->base += (uint64_t)count;
    return NGW_OK;
}

int ngw_key_table_read(ngw_handle* h, ngw_key_table* t, const int32_t* where_dev, int64_t count, int32_t* value_dev, int32_t* tag_dev) {
    if (int rc = valued_call_args(h, t, where_dev, value_dev, tag_dev, count, 0x7FFFFFFFll * NGW_TABLE_BLOCK)) return rc;
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    NgwTableRead x{};
    x.best = best_of(t); x.tag = tag_of(t); x.flags = h->b.flags; x.where = where_dev; x.value = value_dev; x.tag_out = tag_dev;
    x.mask = t->buckets - 1; x.count = count;
    HIP_TRY(ngw_table_read_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_key_table_trace(ngw_handle* h, ngw_key_table* t, const int32_t* where_dev, int64_t count, int32_t steps, int32_t n_actions, int32_t* plans_dev,
                        int32_t* length_dev, int32_t* root_dev) {
    if (int rc = valued_call_args(h, t, where_dev, length_dev, root_dev, count, 0x7FFFFFFFll)) return rc;
    if (steps < 0 || steps > NGW_TRACE_MAX_STEPS) return fail(NGW_E_INVALID_ARG, "ngw_key_table_trace: steps %d outside [0, %d]", steps, NGW_TRACE_MAX_STEPS);
    if (steps > 0 && !plans_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (n_actions < 1) return fail(NGW_E_INVALID_ARG, "ngw_key_table_trace: n_actions %d < 1", n_actions);
    if (t->buckets * (uint64_t)n_actions > 0x7FFFFFFFull)
        return fail(NGW_E_INVALID_ARG, "ngw_key_table_trace: buckets * n_actions = %llu does not fit a tag (at most 2^31 - 1)",
                    (unsigned long long)(t->buckets * (uint64_t)n_actions));
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    NgwTableTrace x{};
    x.key = t->slab; x.tag = tag_of(t); x.flags = h->b.flags; x.where = where_dev; x.plans = plans_dev; x.length = length_dev; x.root = root_dev;
    x.mask = t->buckets - 1; x.count = count; x.T = steps; x.A = n_actions;
    HIP_TRY(ngw_table_trace_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_key_table_lookup(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, int64_t count, int32_t* where_dev) {
    if (int rc = table_call_args(h, t, keys_dev, where_dev, where_dev, count)) return rc;
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    const NgwTable x = table_args(h, t, keys_dev, count, where_dev, nullptr);
    HIP_TRY(ngw_table_lookup_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_key_table_count(ngw_handle* h, ngw_key_table* t, int64_t* n) {
    if (!h || !t || !n) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->tables, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (int rc = enter(h)) return rc;
    unsigned long long stored = 0;
    HIP_TRY(hipMemcpyAsync(&stored, t->slab + 2 * t->buckets, sizeof(stored), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n = (int64_t)stored;
    return NGW_OK;
}

}  // extern "C"
