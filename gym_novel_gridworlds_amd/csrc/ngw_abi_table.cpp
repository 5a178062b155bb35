// ngw_abi_table.cpp - device-side key tables (see ngw_host.h): an open-addressing hash set of 64-bit keys per table, in one allocation of the
// handle, and the kernels (ngw_table.inc) that offer keys to it and look them up.  The calls write no env state: they neither call
// state_written() nor touch anything the handle derives from its state.  Every entry point runs on the handle's stream, behind enter(): a
// table is only ever used in the order of the calls on that one stream (concurrent inserts from two streams are not supported).
#include "ngw_host.h"

using namespace ngwh;

namespace {

// is `t` an open key table of `h`?  (looked up by address, never dereferenced first: a closed one, or another handle's, is simply not found)
bool owns_table(const ngw_handle* h, const ngw_key_table* t) {
    for (const ngw_key_table* q : h->tables)
        if (q == t) return true;
    return false;
}

// key[] zero-filled, stamp[] all ones, the counter 0: the table as it is created, on the handle's stream
int wipe(ngw_handle* h, ngw_key_table* t) {
    const size_t words = (size_t)t->buckets;
    HIP_TRY(hipMemsetAsync(t->slab, 0, words * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->slab + words, 0xFF, words * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->slab + 2 * words, 0, 8, h->stream));
    t->base = 0;
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
    if (!owns_table(h, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (count < 0 || count > 0x7FFFFFFFll * NGW_TABLE_BLOCK) return fail(NGW_E_INVALID_ARG, "key table call with %lld keys", (long long)count);
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_key_table_create(ngw_handle* h, int64_t capacity, ngw_key_table** out) {
    if (!h || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (capacity < 1 || capacity > (1ll << 29)) return fail(NGW_E_INVALID_ARG, "key table capacity %lld outside [1, 2^29]", (long long)capacity);
    if (int rc = enter(h)) return rc;
    uint64_t buckets = 2;
    while (buckets < 2 * (uint64_t)capacity) buckets <<= 1;
    uint64_t* slab = nullptr;
    if (int rc = dev_alloc(h, &slab, (size_t)(2 * buckets + 1))) return rc;      // (zero-filled on the handle's stream)
    ngw_key_table* t = new ngw_key_table;
    t->cap = capacity; t->buckets = buckets; t->slab = slab;
    const hipError_t e = hipMemsetAsync(slab + buckets, 0xFF, (size_t)buckets * 8, h->stream);
    if (e != hipSuccess) {
        dev_free(h, slab);
        delete t;
        return fail(NGW_E_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    h->tables.push_back(t);
    *out = t;
    return NGW_OK;
}

int ngw_key_table_destroy(ngw_handle* h, ngw_key_table* t) {
    if (!h || !t) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!owns_table(h, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
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
    if (!owns_table(h, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
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
    if (!owns_table(h, t)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    if (int rc = enter(h)) return rc;
    unsigned long long stored = 0;
    HIP_TRY(hipMemcpyAsync(&stored, t->slab + 2 * t->buckets, sizeof(stored), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n = (int64_t)stored;
    return NGW_OK;
}

}  // extern "C"
