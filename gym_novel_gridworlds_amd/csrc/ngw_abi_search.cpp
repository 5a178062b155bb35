// ngw_abi_search.cpp - search runs (see ngw_host.h): whole best-first iterations over one snapshot pool and one valued key table, enqueued from one
// call.  The driver owns no stage of its own: successor keys, insert_min, compaction / selection, slot allocation and expand run through their own
// entry points (ngw_abi_snapshot.cpp, ngw_abi_table.cpp, ngw_abi_frontier.cpp), called as any caller calls them, with the three kernels of
// ngw_search.inc between them.  The calls write no env state: they neither call state_written() nor touch anything the handle derives from its
// state.  All run on the handle's stream, behind enter(); only ngw_search_read / _read_open wait.  An open-list search (ngw_search_create_open) adds
// the selection over f in front, the walk of the children behind, and the take and open kernels; the same driver serves it.  The recipe term
// (ngw_search_set_recipe) is one launch more in front of the open and the roots kernel, recipe_run of ngw_abi_recipe.cpp; a search without the term
// enqueues exactly what it always did.
#include "ngw_host.h"

using namespace ngwh;

namespace {

// The stats ring holds one row more than ngw_search_read reports: the settle kernel of iteration i zero-fills the row of iteration i + 1, which in a
// ring of NGW_SEARCH_ROWS rows would be the row of iteration i + 1 - NGW_SEARCH_ROWS - the oldest of the rows still to be reported.
constexpr int64_t SEARCH_RING = NGW_SEARCH_ROWS + 1;

// the pool and the table of a search are still open on `h` (by address: a closed one is simply not found)
bool parts_open(const ngw_handle* h, const ngw_snapshot* pool, const ngw_key_table* table) { return is_open(h->snaps, pool) && is_open(h->tables, table); }

int search_call_args(const ngw_handle* h, const ngw_search* s) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->searches, s)) return fail(NGW_E_INVALID_ARG, "not an open search of this handle");
    if (!parts_open(h, s->pool, s->table)) return fail(NGW_E_INVALID_ARG, "the search's snapshot or key table is closed");
    return NGW_OK;
}

// the arguments the three kernels share, for iteration s->iterations
NgwSearch search_args(const ngw_search* s) {
    NgwSearch x{};
    x.parents = s->parents[s->cur]; x.next = s->parents[s->cur ^ 1]; x.g = s->g; x.bucket = s->bucket;
    x.info = reinterpret_cast<const uint32_t*>(s->info); x.lut = s->lut; x.values = s->values; x.tags = s->tags; x.where = s->where; x.best = s->best;
    x.first = s->first; x.second = s->second; x.slots = s->slots; x.plist = s->plist;
    x.goal = s->goal; x.overflowed = s->goal + 1;
    x.row = s->stats + 4 * (s->iterations % SEARCH_RING); x.next_row = s->stats + 4 * ((s->iterations + 1) % SEARCH_RING);
    x.capacity = s->cap; x.pool = s->pool_cap; x.A = s->A; x.by_action = s->by_action; x.stop = s->stop;
    if (s->open) {
        x.f = s->f; x.h = s->h; x.slot_of_bucket = s->slot_of_bucket; x.dist = s->dist; x.weights = s->weights; x.sel_count = s->count;
        x.orow = s->ostats + NGW_SEARCH_OPEN_COLS * (s->iterations % SEARCH_RING); x.next_orow = s->ostats + NGW_SEARCH_OPEN_COLS * ((s->iterations + 1) % SEARCH_RING);
        x.buckets = s->buckets; x.K = s->K; x.mode = s->hmode; x.prune = s->prune;
        x.recipe = s->recipe;
    }
    return x;
}

// one iteration: ngw.h's seven steps in their order; an open-list search: its steps 0 to 8
int iterate(ngw_handle* h, ngw_search* s) {
    const NgwSearch x = search_args(s);
    if (s->open) {                                    // step 0: the `keep` smallest f of the whole pool are the parents, closed by the take
        if (int rc = ngw_frontier_select(h, s->f, nullptr, s->pool_cap, 1, 1, nullptr, s->keep, 0, s->cap, s->parents[s->cur], nullptr, s->taken, s->bound, s->count))
            return rc;
        HIP_TRY(ngw_search_take_launch(&x, h->stream));
    }
    if (int rc = ngw_successor_keys(h, s->pool, x.parents, s->cap, NGW_KEY_STATE, s->keys, nullptr, nullptr, reinterpret_cast<uint32_t*>(s->info))) return rc;
    HIP_TRY(ngw_search_offer_launch(&x, h->stream));
    if (int rc = ngw_key_table_insert_min(h, s->table, s->keys, s->values, s->tags, s->n, s->where, s->fresh, s->best)) return rc;
    HIP_TRY(ngw_search_judge_launch(&x, h->stream));
    if (s->keep < 0 || s->open) {                     // (an open-list search chose in step 0: every improved child is kept)
        if (int rc = ngw_frontier_compact(h, s->best, s->n, s->A, nullptr, s->cap, s->first, s->second, s->count)) return rc;
    } else {
        if (int rc = ngw_frontier_select(h, s->values, s->best, s->n, 1, s->A, nullptr, s->keep, 0, s->cap, s->first, s->second, s->taken, s->bound, s->count))
            return rc;
    }
    if (int rc = ngw_frontier_alloc(h, s->count, s->cursor, (int32_t)s->pool_cap, s->cap, s->slots)) return rc;
    HIP_TRY(ngw_search_settle_launch(&x, h->stream));
    if (int rc = ngw_snapshot_expand(h, s->pool, s->plist, s->second, s->pool, s->slots, s->cap, nullptr, nullptr, nullptr)) return rc;
    if (s->open) {                                    // step 8: the children join the open list
        if (s->dist)
            if (int rc = ngw_snapshot_walk(h, s->pool, x.next, s->cap, nullptr, 0, s->dist, nullptr, nullptr)) return rc;
        if (s->recipe)                                // (the recipe term of the same list: a padded entry gives 0 and no flag)
            if (int rc = recipe_run(h, s->pool->r, s->pool->cap, x.next, s->cap, s->recipe_prog, s->recipe)) return rc;
        HIP_TRY(ngw_search_open_launch(&x, h->stream));
    }
    s->cur ^= 1;
    s->iterations++;
    return NGW_OK;
}

// ngw_search_create and ngw_search_create_open: the checks, the ONE allocation and its initial contents
int create(ngw_handle* h, ngw_snapshot* pool, ngw_key_table* table, const ngw_search_options& o, bool open, ngw_search_arrays* arrays, ngw_search_arrays_open* more,
           ngw_search** out) {
    const int64_t capacity = o.capacity;
    const int32_t keep = o.keep;
    *out = nullptr;
    if (!parts_open(h, pool, table)) return fail(NGW_E_INVALID_ARG, "not an open snapshot and an open key table of this handle");
    if (!table->valued) return fail(NGW_E_INVALID_ARG, "a key table without values (ngw_key_table_create_valued makes one with)");
    const int64_t A = h->spec.n_actions;
    if (capacity < 1 || capacity > pool->cap) return fail(NGW_E_INVALID_ARG, "search capacity %lld outside [1, the pool's %lld]", (long long)capacity, (long long)pool->cap);
    if (capacity * A > NGW_FRONTIER_MAX_FLAGS)
        return fail(NGW_E_INVALID_ARG, "search capacity %lld: %lld positions in one iteration (at most 2^24)", (long long)capacity, (long long)(capacity * A));
    if (pool->cap > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "a pool of %lld slots", (long long)pool->cap);
    if ((int64_t)keep > capacity) return fail(NGW_E_INVALID_ARG, "keep: %d entries do not fit the capacity %lld", (int)keep, (long long)capacity);
    const int32_t K = h->proto.K;
    if (open) {
        if (keep < 1) return fail(NGW_E_INVALID_ARG, "keep: an open-list search expands keep >= 1 states per iteration, got %d", (int)keep);
        if (pool->cap > NGW_SELECT_MAX_VALUES)
            return fail(NGW_E_INVALID_ARG, "an open-list search chooses among every slot: a pool of %lld slots (at most 2^24)", (long long)pool->cap);
        if (o.heuristic != NGW_SEARCH_H_NONE && o.heuristic != NGW_SEARCH_H_MIN && o.heuristic != NGW_SEARCH_H_MAX)
            return fail(NGW_E_INVALID_ARG, "heuristic mode %d (NGW_SEARCH_H_NONE, _MIN or _MAX)", (int)o.heuristic);
        if (o.heuristic != NGW_SEARCH_H_NONE) {
            if (!o.weights_host) return fail(NGW_E_INVALID_ARG, "NULL argument");
            if (o.n_weights != K) return fail(NGW_E_INVALID_ARG, "heuristic weights: %d given, one per item id (%d) expected", (int)o.n_weights, (int)K);
            for (int32_t k = 0; k < K; k++)
                if (o.weights_host[k] < 0) return fail(NGW_E_INVALID_ARG, "heuristic weights: weight %d is negative (%d)", (int)k, (int)o.weights_host[k]);
        }
    }
    const bool walk = open && o.heuristic != NGW_SEARCH_H_NONE;
    if (table->buckets * (uint64_t)A > 0x7FFFFFFFull)
        return fail(NGW_E_INVALID_ARG, "search: buckets * n_actions = %llu does not fit a tag (at most 2^31 - 1)", (unsigned long long)(table->buckets * (uint64_t)A));
    const size_t lds = NGW_SUCC_LDS_BYTES(h->proto.MS, h->proto.KP);
    if (lds > NGW_SUCC_LDS_MAX)
        return fail(NGW_E_INVALID_ARG, "map_size %d: a search keeps two sets of a wavefront's 64 maps in LDS (ngw_successor_keys) and they need %zu B, more "
                                       "than 160 KiB", h->proto.S, lds);
    if (int rc = enter(h)) return rc;
    const size_t cap = (size_t)capacity, n = cap * (size_t)A, pc = (size_t)pool->cap, nb = (size_t)table->buckets;
    ngw_search* s = new ngw_search;
    s->pool = pool; s->table = table; s->cap = capacity; s->pool_cap = pool->cap; s->n = (int64_t)n;
    s->A = (int32_t)A; s->by_action = o.by_action != 0; s->keep = keep < 0 ? -1 : keep; s->stop = o.stop_at_goals != 0;
    s->open = open; s->prune = o.prune != 0; s->hmode = walk ? o.heuristic : NGW_SEARCH_H_NONE; s->K = K; s->buckets = (int64_t)nb;
    auto layout = [&](Carver c) {                      // the slab, described once: 64-bit words, the int32 arrays, an open-list search's own, the two flag arrays
        s->goal = c.take<unsigned long long>(2); s->keys = c.take<uint64_t>(n);                                      // goal, overflowed | keys
        s->stats = c.take<uint32_t>(4 * SEARCH_RING); s->lut = c.take<int32_t>(64);
        s->cursor = c.take<int32_t>(1); s->count = c.take<int32_t>(2); s->taken = c.take<int32_t>(1); s->bound = c.take<int32_t>(1); c.take<int32_t>(3);   // (3 spare)
        s->parents[0] = c.take<int32_t>(cap); s->parents[1] = c.take<int32_t>(cap); s->first = c.take<int32_t>(cap); s->second = c.take<int32_t>(cap);
        s->slots = c.take<int32_t>(cap); s->plist = c.take<int32_t>(cap); s->g = c.take<int32_t>(pc); s->bucket = c.take<int32_t>(pc);
        s->info = c.take<int32_t>(n); s->values = c.take<int32_t>(n); s->tags = c.take<int32_t>(n); s->where = c.take<int32_t>(n);
        if (open) {
            c.align(16);                                                           // the weights and the distances start on 16 bytes
            if (walk) { s->weights = c.take<int32_t>(((size_t)K + 3) & ~(size_t)3); s->dist = c.take<int32_t>(cap * (size_t)K); }
            s->ostats = c.take<uint32_t>((size_t)NGW_SEARCH_OPEN_COLS * SEARCH_RING);
            s->h = c.take<int32_t>(pc); s->f = c.take<int32_t>(pc); s->slot_of_bucket = c.take<int32_t>(nb);
        }
        c.align(8);
        s->fresh = c.take<uint8_t>(n); s->best = c.take<uint8_t>(n); c.align(8);
        return c.bytes;
    };
    uint64_t* slab = nullptr;
    if (int rc = dev_alloc(h, &slab, layout(Carver()) / 8)) { delete s; return rc; }   // (zero-filled on the handle's stream)
    layout(Carver(slab));
    s->slab = slab;
    hipError_t e = hipMemsetAsync(s->goal, 0xFF, 8, h->stream);                                                   // no goal yet
    if (e == hipSuccess) e = hipMemcpyAsync(s->lut, o.costs_host, 64 * sizeof(int32_t), hipMemcpyDefault, h->stream);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->parents[0]), (int)NGW_IDX_NONE, 2 * cap, h->stream);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->g), NGW_VALUE_NONE, pc, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->bucket, 0xFF, pc * sizeof(int32_t), h->stream);                    // -1: no bucket
    int32_t first_row[NGW_SEARCH_OPEN_COLS] = {0};                                                                // no slot chosen yet: the take's min / max words
    first_row[NGW_SEARCH_FMIN] = NGW_VALUE_NONE; first_row[NGW_SEARCH_FBOUND] = INT32_MIN;
    if (open) {
        if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->f), NGW_VALUE_NONE, pc, h->stream);                        // nothing is open
        if (e == hipSuccess) e = hipMemsetAsync(s->slot_of_bucket, 0xFF, nb * sizeof(int32_t), h->stream);                                         // -1: no slot
        if (e == hipSuccess) e = hipMemcpyAsync(s->ostats, first_row, sizeof(first_row), hipMemcpyDefault, h->stream);
        if (e == hipSuccess && walk) e = hipMemcpyAsync(s->weights, o.weights_host, (size_t)K * sizeof(int32_t), hipMemcpyDefault, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);                                                     // (the host arrays are the caller's: read by now)
    if (e != hipSuccess) {
        dev_free(h, slab);
        delete s;
        return fail(NGW_E_HIP, "search setup failed: %s", hipGetErrorString(e));
    }
    h->searches.push_back(s);
    arrays->parents[0] = s->parents[0]; arrays->parents[1] = s->parents[1]; arrays->g = s->g; arrays->bucket = s->bucket; arrays->cursor = s->cursor;
    if (more) { more->h = s->h; more->f = s->f; }
    *out = s;
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_search_create(ngw_handle* h, ngw_snapshot* pool, ngw_key_table* table, int64_t capacity, const int32_t* costs_host, int32_t by_action, int32_t keep,
                      int32_t stop_at_goals, ngw_search_arrays* arrays, ngw_search** out) {
    if (!h || !pool || !table || !costs_host || !arrays || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    ngw_search_options o{};
    o.capacity = capacity; o.costs_host = costs_host; o.by_action = by_action; o.keep = keep; o.stop_at_goals = stop_at_goals;
    return create(h, pool, table, o, false, arrays, nullptr, out);
}

int ngw_search_create_open(ngw_handle* h, ngw_snapshot* pool, ngw_key_table* table, const ngw_search_options* options, ngw_search_arrays_open* arrays,
                           ngw_search** out) {
    if (!h || !pool || !table || !options || !options->costs_host || !arrays || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    return create(h, pool, table, *options, true, &arrays->base, arrays, out);
}

int ngw_search_destroy(ngw_handle* h, ngw_search* s) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->searches, s)) return fail(NGW_E_INVALID_ARG, "not an open search of this handle");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                         // (queued iterations may still use the arrays)
    for (size_t i = 0; i < h->searches.size(); i++)
        if (h->searches[i] == s) { h->searches.erase(h->searches.begin() + (long)i); break; }
    dev_free(h, s->slab);
    if (s->recipe) dev_free(h, s->recipe);
    delete s;
    return NGW_OK;
}

int ngw_search_set_recipe(ngw_handle* h, ngw_search* s, const ngw_recipe_program* program) {
    if (int rc = search_call_args(h, s)) return rc;
    if (!program) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!s->open) return fail(NGW_E_INVALID_ARG, "a search without an open list has no heuristic (ngw_search_create_open makes one with)");
    if (s->started || s->iterations) return fail(NGW_E_INVALID_ARG, "ngw_search_set_recipe is legal only before ngw_search_start");
    if (int rc = enter(h)) return rc;
    NgwRecipeProg prog;
    if (int rc = recipe_pack(h, program, &prog)) return rc;
    if (!s->recipe)
        if (int rc = dev_alloc(h, &s->recipe, (size_t)s->cap)) return rc;         // (zero-filled on the handle's stream; ngw_search_run allocates nothing)
    s->recipe_prog = prog;
    return NGW_OK;
}

int ngw_search_start(ngw_handle* h, ngw_search* s, const int32_t* roots_dev, int64_t count, int32_t* current) {
    if (int rc = search_call_args(h, s)) return rc;
    if (count < 0 || count > s->cap) return fail(NGW_E_INVALID_ARG, "%lld roots in a search of capacity %lld", (long long)count, (long long)s->cap);
    if (count && !roots_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    s->started = true;
    if (count) {
        // the scratch of an iteration serves: values 0, tags NGW_TAG_ROOT; the values the table holds afterwards go to `info`, their tags to `plist`
        HIP_TRY(hipMemsetAsync(s->values, 0, (size_t)count * sizeof(int32_t), h->stream));
        HIP_TRY(hipMemsetAsync(s->tags, 0xFF, (size_t)count * sizeof(int32_t), h->stream));
        if (int rc = ngw_state_keys(h, s->pool, roots_dev, count, NGW_KEY_STATE, s->keys)) return rc;
        if (int rc = ngw_key_table_insert_min(h, s->table, s->keys, s->values, s->tags, count, s->where, s->fresh, s->best)) return rc;
        if (int rc = ngw_key_table_read(h, s->table, s->where, count, s->info, s->plist)) return rc;
    }
    NgwSearchRoots x{};
    x.roots = roots_dev; x.where = s->where; x.value = s->info; x.best = s->best; x.parents = s->parents[s->cur]; x.g = s->g; x.bucket = s->bucket;
    x.count = count; x.capacity = s->cap; x.pool = s->pool_cap;
    if (s->open) {                                    // the roots are opened, not made parents: the first iteration chooses them
        if (count && s->dist)
            if (int rc = ngw_snapshot_walk(h, s->pool, roots_dev, count, nullptr, 0, s->dist, nullptr, nullptr)) return rc;
        x.f = s->f; x.h = s->h; x.slot_of_bucket = s->slot_of_bucket; x.dist = s->dist; x.weights = s->weights; x.buckets = s->buckets; x.K = s->K; x.mode = s->hmode;
        if (s->recipe) {
            if (count)
                if (int rc = recipe_run(h, s->pool->r, s->pool->cap, roots_dev, count, s->recipe_prog, s->recipe)) return rc;
            x.recipe = s->recipe;
        }
    }
    HIP_TRY(ngw_search_roots_launch(&x, h->stream));
    if (current) *current = s->cur;
    return NGW_OK;
}

int ngw_search_run(ngw_handle* h, ngw_search* s, int32_t iterations, int32_t* current) {
    if (int rc = search_call_args(h, s)) return rc;
    if (iterations < 0) return fail(NGW_E_INVALID_ARG, "%d iterations", (int)iterations);
    if (int rc = enter(h)) return rc;
    int rc = NGW_OK;
    for (int32_t i = 0; i < iterations && rc == NGW_OK; i++) rc = iterate(h, s);
    if (current) *current = s->cur;
    return rc;
}

int ngw_search_read(ngw_handle* h, ngw_search* s, ngw_search_report* out) {
    if (!h || !s || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->searches, s)) return fail(NGW_E_INVALID_ARG, "not an open search of this handle");
    if (int rc = enter(h)) return rc;
    uint64_t head[2] = {0, 0};
    uint32_t ring[SEARCH_RING][4];
    int32_t cursor = 0;
    uint32_t flags = 0;
    HIP_TRY(hipMemcpyAsync(head, s->slab, sizeof(head), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(ring, s->stats, sizeof(ring), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(&cursor, s->cursor, sizeof(cursor), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(&flags, h->b.flags, sizeof(flags), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->b.flags_host) flags |= *h->b.flags_host;
    memset(out, 0, sizeof(*out));
    out->iterations = s->iterations;
    out->overflowed = head[1];
    out->goal_value = (int32_t)((uint32_t)(head[0] >> 32) ^ 0x80000000u);
    out->goal_bucket = (int32_t)(uint32_t)head[0];
    out->cursor = cursor;
    out->flags = flags;
    out->rows = (int32_t)(s->iterations < NGW_SEARCH_ROWS ? s->iterations : NGW_SEARCH_ROWS);
    out->current = s->cur;
    for (int32_t i = 0; i < out->rows; i++)
        memcpy(out->stats[i], ring[(s->iterations - out->rows + i) % SEARCH_RING], sizeof(ring[0]));
    return NGW_OK;
}

int ngw_search_read_open(ngw_handle* h, ngw_search* s, ngw_search_open_report* out) {
    if (!h || !s || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->searches, s)) return fail(NGW_E_INVALID_ARG, "not an open search of this handle");
    if (!s->open) return fail(NGW_E_INVALID_ARG, "a search without an open list (ngw_search_create_open makes one with)");
    if (int rc = enter(h)) return rc;
    uint32_t ring[SEARCH_RING][NGW_SEARCH_OPEN_COLS];
    HIP_TRY(hipMemcpyAsync(ring, s->ostats, sizeof(ring), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    memset(out, 0, sizeof(*out));
    out->iterations = s->iterations;
    out->rows = (int32_t)(s->iterations < NGW_SEARCH_ROWS ? s->iterations : NGW_SEARCH_ROWS);
    for (int32_t i = 0; i < out->rows; i++) {
        const uint32_t* r = ring[(s->iterations - out->rows + i) % SEARCH_RING];
        const bool any = r[NGW_SEARCH_CHOSEN] != 0;
        out->stats[i][0] = (int32_t)r[NGW_SEARCH_CHOSEN]; out->stats[i][1] = (int32_t)r[NGW_SEARCH_PRUNED]; out->stats[i][2] = (int32_t)r[NGW_SEARCH_SUPERSEDED];
        out->stats[i][3] = (int32_t)r[NGW_SEARCH_OPEN];
        out->stats[i][4] = any ? (int32_t)r[NGW_SEARCH_FMIN] : NGW_VALUE_NONE;
        out->stats[i][5] = any ? (int32_t)r[NGW_SEARCH_FBOUND] : NGW_VALUE_NONE;
    }
    return NGW_OK;
}

}  // extern "C"
