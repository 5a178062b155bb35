// ngw_abi_tree.cpp - tree-search runs (see ngw_host.h): whole MCTS iterations over one key table, enqueued from one call.  The
// driver owns no stage of the playout or the table: the guided playout, the insert, the state keys and the mask words run through their own entry
// points (ngw_abi_snapshot.cpp, ngw_abi_table.cpp), called as any caller calls them, with the kernels of ngw_tree.inc between them.  The
// calls write no env state: they neither call state_written() nor touch anything the handle derives from its state.  All run on the handle's
// stream, behind enter(); only ngw_tree_report waits.
#include "ngw_host.h"

using namespace ngwh;

namespace {

// The stats ring holds one row more than ngw_tree_report reports: the leaf kernel of iteration i zero-fills the row of iteration i + 1, which in a
// ring of NGW_TREE_ROWS rows would be the oldest of the rows still to be reported (as in ngw_abi_search.cpp).
constexpr uint64_t TREE_RING = NGW_TREE_ROWS + 1;

int tree_call_args(const ngw_handle* h, const ngw_tree* t) {
    if (!h || !t) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->trees, t)) return fail(NGW_E_INVALID_ARG, "not an open tree search of this handle");
    if (!is_open(h->tables, t->table)) return fail(NGW_E_INVALID_ARG, "the tree search's key table is closed");
    return NGW_OK;
}

// the table and the source of the roots are still open on `h` (by address: a closed one is simply not found)
int run_parts(const ngw_handle* h, const ngw_tree* t) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (t->src && !is_open(h->snaps, t->src)) return fail(NGW_E_INVALID_ARG, "the snapshot of the tree search's roots is closed");
    return NGW_OK;
}

// what the kernels share: the statistics and the sizes
NgwTree tree_args(const ngw_handle* h, const ngw_tree* t) {
    NgwTree x{};
    x.visits = t->visits; x.returns = t->returns; x.mask_words = t->mask_words; x.rows = t->rows; x.priors = t->priors;
    x.leaf_keys = t->leaf_keys; x.leaf_masks = t->leaf_masks; x.where_leaf = t->where_leaf; x.fresh = t->fresh; x.touched = t->touched;
    x.flags = h->b.flags;
    x.cap = t->cap; x.buckets = t->buckets; x.T = t->T; x.n = t->T; x.A = t->A; x.combine = t->combine; x.c = t->c; x.q_init = t->q_init;
    return x;
}

// ... and the recorded arrays of the tree's own playout, with this iteration's stats rows
NgwTree run_args(const ngw_handle* h, const ngw_tree* t) {
    NgwTree x = tree_args(h, t);
    x.actions = t->actions; x.rewards = t->rewards; x.where = t->where; x.depth = t->depth; x.length = t->length; x.keys = t->keys; x.masks = t->masks;
    x.count = t->n_roots; x.stride = t->cap;
    x.row = t->stats + NGW_TREE_COLS * (t->iterations % TREE_RING); x.next_row = t->stats + NGW_TREE_COLS * ((t->iterations + 1) % TREE_RING);
    return x;
}

int playout(ngw_handle* h, ngw_tree* t, int64_t count, uint64_t seed, uint64_t first_pair) {
    return ngw_snapshot_playout_guided(h, t->src, t->roots, count, t->T, seed, first_pair, t->weights, nullptr, nullptr, nullptr, t->ret, t->length, t->ended,
                                       t->info, t->first_action, t->actions, t->cap, t->fields, t->keys, t->cap, t->rewards, t->cap, t->masks, t->cap, nullptr, 0,
                                       nullptr, t->table, t->rows, t->where, t->cap, t->depth, NGW_OUTSIDE_DEFAULT);
}

// steps 2 and 3 of include/ngw.h over x's recorded arrays
int grow(ngw_handle* h, ngw_tree* t, const NgwTree& x) {
    HIP_TRY(ngw_tree_leaf_launch(&x, h->stream));
    if (int rc = ngw_key_table_insert(h, t->table, t->leaf_keys, x.count, t->where_leaf, t->fresh)) return rc;
    HIP_TRY(ngw_tree_grow_launch(&x, h->stream));
    return NGW_OK;
}

// rule 4: the undiscounted kernel, or under a discount its twin
int backup(ngw_handle* h, const ngw_tree* t, const NgwTree& x) {
    const NgwTreeRule rule{t->spread, t->discount_q16};
    if (t->discount_q16 != 65536) HIP_TRY(ngw_tree_backup_discount_launch(&x, &rule, h->stream));
    else HIP_TRY(ngw_tree_backup_launch(&x, h->stream));
    return NGW_OK;
}

// rule 5: the one-lane kernel, or the 16-lane form - for every spread above 1, and at spread 1 where the rule asks for it (rows16 = 1)
int reweight(ngw_handle* h, const ngw_tree* t, NgwTree x, const int32_t* list, int64_t n) {
    x.list = list; x.n_list = n;
    const NgwTreeRule rule{t->spread, t->discount_q16};
    if (t->spread > 1 || t->rows16 == 1) HIP_TRY(ngw_tree_reweight16_launch(&x, &rule, h->stream));
    else HIP_TRY(ngw_tree_reweight_launch(&x, h->stream));
    return NGW_OK;
}

// one iteration: ngw.h's five steps in their order
int iterate(ngw_handle* h, ngw_tree* t, uint64_t seed) {
    const NgwTree x = run_args(h, t);
    if (int rc = playout(h, t, t->n_roots, seed, t->iterations * (uint64_t)t->cap)) return rc;
    if (int rc = grow(h, t, x)) return rc;
    if (int rc = backup(h, t, x)) return rc;
    if (int rc = reweight(h, t, x, t->touched, (int64_t)t->T * t->cap)) return rc;
    t->iterations++;
    return NGW_OK;
}

int zero_statistics(ngw_handle* h, ngw_tree* t) {
    const size_t n = (size_t)t->buckets * (size_t)t->A;
    HIP_TRY(hipMemsetAsync(t->returns, 0, n * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->mask_words, 0, (size_t)t->buckets * 8, h->stream));
    HIP_TRY(hipMemsetAsync(t->visits, 0, n * 4, h->stream));
    HIP_TRY(hipMemsetAsync(t->rows, 0, n * 4, h->stream));
    HIP_TRY(hipMemsetAsync(t->stats, 0, TREE_RING * NGW_TREE_COLS * 4, h->stream));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t->roots), (int)NGW_IDX_NONE, (size_t)t->cap, h->stream));
    HIP_TRY(hipMemsetAsync(t->touched, 0xFF, (size_t)t->T * (size_t)t->cap * 4, h->stream));       // -1: nothing touched
    HIP_TRY(hipMemsetAsync(t->where_leaf, 0xFF, (size_t)t->cap * 4, h->stream));
    t->iterations = 0;
    t->n_roots = 0;
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_tree_create(ngw_handle* h, ngw_key_table* table, const ngw_tree_options* o, ngw_tree** out) {
    if (!h || !table || !o || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (!is_open(h->tables, table)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
    const int64_t A = h->spec.n_actions, P = o->playouts, T = o->steps;
    if (P < 1) return fail(NGW_E_INVALID_ARG, "tree search: %lld playouts per iteration", (long long)P);
    if (T < 1) return fail(NGW_E_INVALID_ARG, "tree search: playouts of %lld steps", (long long)T);
    if (P > 0x7FFFFFFFll || P * T > 0x7FFFFFFFll)
        return fail(NGW_E_INVALID_ARG, "tree search: playouts * steps = %lld * %lld recorded entries per iteration (at most 2^31 - 1)", (long long)P, (long long)T);
    if (table->buckets * (uint64_t)A > 0x7FFFFFFFull)
        return fail(NGW_E_INVALID_ARG, "tree search: buckets * n_actions = %llu entries of statistics (at most 2^31 - 1)", (unsigned long long)(table->buckets * (uint64_t)A));
    if (o->fields == 0 || (o->fields & ~NGW_KEY_ALL)) return fail(NGW_E_INVALID_ARG, "tree search: fields 0x%x: a non-empty selection of NGW_KEY_* bits expected", (unsigned)o->fields);
    if (!std::isfinite(o->c) || !std::isfinite(o->q_init)) return fail(NGW_E_INVALID_ARG, "tree search: c = %g, q_init = %g: finite values expected", (double)o->c, (double)o->q_init);
    if (int rc = enter(h)) return rc;
    const size_t p = (size_t)P, tp = (size_t)(P * T), nb = (size_t)table->buckets, na = nb * (size_t)A, a = (size_t)A;
    ngw_tree* t = new ngw_tree;
    t->table = table; t->cap = P; t->buckets = (int64_t)nb; t->T = (int32_t)T; t->A = (int32_t)A; t->fields = o->fields; t->c = o->c; t->q_init = o->q_init;
    t->combine = o->plain_backup == 0;
    float* weights = nullptr;
    auto layout = [&](Carver c) {                       // the slab, described once: the 64-bit words, the 32-bit arrays, the bytes
        t->returns = c.take<unsigned long long>(na); t->mask_words = c.take<uint64_t>(nb);
        t->keys = c.take<uint64_t>(tp); t->masks = c.take<uint64_t>(tp); t->leaf_keys = c.take<uint64_t>(p); t->leaf_masks = c.take<uint64_t>(p);
        t->visits = c.take<int32_t>(na); t->rows = c.take<float>(na);
        if (o->priors) t->priors = c.take<float>(na);
        t->actions = c.take<int32_t>(tp); t->rewards = c.take<int32_t>(tp); t->where = c.take<int32_t>(tp); t->touched = c.take<int32_t>(tp);
        t->depth = c.take<int32_t>(p); t->length = c.take<int32_t>(p); t->ret = c.take<int32_t>(p); t->first_action = c.take<int32_t>(p);
        t->where_leaf = c.take<int32_t>(p); t->roots = c.take<int32_t>(p); t->start_actions = c.take<int32_t>(p); t->info = c.take<uint32_t>(p);
        t->zero_weights = c.take<float>(a * p); weights = c.take<float>((a + 1) & ~(size_t)1);      // weights: [A], an even number of words
        t->stats = c.take<uint32_t>(TREE_RING * NGW_TREE_COLS); c.align(8);
        t->ended = c.take<uint8_t>(p); t->fresh = c.take<uint8_t>(p); c.align(8);
        return c.bytes;
    };
    uint64_t* slab = nullptr;
    if (int rc = dev_alloc(h, &slab, layout(Carver()) / 8)) { delete t; return rc; }      // (zero-filled on the handle's stream)
    layout(Carver(slab));
    t->slab = slab;
    h->trees.push_back(t);                                            // (listed before the first call that looks it up)
    int rc = zero_statistics(h, t);
    if (rc == NGW_OK && o->weights_host) {
        t->weights = weights;
        hipError_t e = hipMemcpyAsync(weights, o->weights_host, a * sizeof(float), hipMemcpyDefault, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);    // (the host array is the caller's: read by now)
        if (e != hipSuccess) rc = fail(NGW_E_HIP, "tree search setup failed: %s", hipGetErrorString(e));
    }
    if (rc == NGW_OK) rc = playout(h, t, 0, 0, 0);                    // (a call of no pairs makes every check of the guided playout: the map-size limit above all)
    if (rc != NGW_OK) {
        h->trees.pop_back();
        (void)hipStreamSynchronize(h->stream);
        dev_free(h, slab);
        delete t;
        return rc;
    }
    *out = t;
    return NGW_OK;
}

int ngw_tree_destroy(ngw_handle* h, ngw_tree* t) {
    if (!h || !t) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->trees, t)) return fail(NGW_E_INVALID_ARG, "not an open tree search of this handle");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                         // (queued iterations may still use the arrays)
    for (size_t i = 0; i < h->trees.size(); i++)
        if (h->trees[i] == t) { h->trees.erase(h->trees.begin() + (long)i); break; }
    dev_free(h, t->slab);
    delete t;
    return NGW_OK;
}

int ngw_tree_arrays(ngw_handle* h, ngw_tree* t, ngw_tree_device_arrays* out) {
    if (!h || !t || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->trees, t)) return fail(NGW_E_INVALID_ARG, "not an open tree search of this handle");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                         // (the arrays are the caller's to read and write from here on: their zero-fill has run)
    memset(out, 0, sizeof(*out));
    out->visits = t->visits; out->returns = t->returns; out->mask_words = t->mask_words; out->rows = t->rows; out->priors = t->priors;
    out->roots = t->roots; out->actions = t->actions; out->keys = t->keys; out->rewards = t->rewards; out->masks = t->masks; out->where = t->where;
    out->depth = t->depth; out->length = t->length; out->ret = t->ret; out->ended = t->ended; out->info = t->info;
    out->leaf_keys = t->leaf_keys; out->leaf_masks = t->leaf_masks; out->where_leaf = t->where_leaf; out->fresh = t->fresh; out->touched = t->touched;
    out->buckets = t->buckets; out->n_actions = t->A;
    return NGW_OK;
}

int ngw_tree_start(ngw_handle* h, ngw_tree* t, ngw_snapshot* src, const int32_t* roots_dev, int64_t count) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (src && !is_open(h->snaps, src)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (count < 0 || count > t->cap) return fail(NGW_E_INVALID_ARG, "%lld roots in a tree search of %lld playouts", (long long)count, (long long)t->cap);
    if (count && !roots_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t->roots), (int)NGW_IDX_NONE, (size_t)t->cap, h->stream));
    t->src = src; t->n_roots = count;
    if (!count) return NGW_OK;
    HIP_TRY(hipMemcpyAsync(t->roots, roots_dev, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    // the scratch of an iteration serves: the roots' keys and mask words in the leaves' place, then the insert, the grow and the reweight of an iteration
    if (int rc = ngw_state_keys(h, src, t->roots, count, t->fields, t->leaf_keys)) return rc;
    if (int rc = ngw_sample_actions(h, src, t->roots, count, t->zero_weights, t->cap, 0, 0, 0, t->start_actions, nullptr, t->leaf_masks)) return rc;
    if (int rc = ngw_key_table_insert(h, t->table, t->leaf_keys, count, t->where_leaf, t->fresh)) return rc;
    NgwTree x = tree_args(h, t);
    x.count = count; x.stride = t->cap;
    HIP_TRY(ngw_tree_grow_launch(&x, h->stream));
    return reweight(h, t, x, t->where_leaf, count);
}

int ngw_tree_run(ngw_handle* h, ngw_tree* t, int32_t iterations, uint64_t seed) {
    if (int rc = run_parts(h, t)) return rc;
    if (iterations < 0) return fail(NGW_E_INVALID_ARG, "%d iterations", (int)iterations);
    if (int rc = enter(h)) return rc;
    for (int32_t i = 0; i < iterations; i++) {
        if (i)                                                        // (the parts are looked up before every iteration, as the search driver does)
            if (int rc = run_parts(h, t)) return rc;
        if (int rc = iterate(h, t, seed)) return rc;
    }
    return NGW_OK;
}

static int stage_args(const ngw_tree* t, int64_t stride, int64_t count, int32_t n_steps) {
    if (count < 0 || count > t->cap) return fail(NGW_E_INVALID_ARG, "%lld pairs in a tree search of %lld playouts", (long long)count, (long long)t->cap);
    if (n_steps < 1 || n_steps > t->T) return fail(NGW_E_INVALID_ARG, "playouts of %d steps in a tree search of %d", (int)n_steps, (int)t->T);
    if (stride < count) return fail(NGW_E_INVALID_ARG, "%lld pairs with a stride of %lld", (long long)count, (long long)stride);
    return NGW_OK;
}

int ngw_tree_grow(ngw_handle* h, ngw_tree* t, const int32_t* depth_dev, const int32_t* length_dev, const uint64_t* keys_dev, const uint64_t* masks_dev, int64_t stride,
                  int64_t count, int32_t n_steps) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (int rc = stage_args(t, stride, count, n_steps)) return rc;
    if (count && (!depth_dev || !length_dev || !keys_dev || !masks_dev)) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipMemsetAsync(t->where_leaf, 0xFF, (size_t)t->cap * 4, h->stream));                    // (the entries behind `count`: no leaf)
    if (!count) return NGW_OK;
    NgwTree x = tree_args(h, t);
    x.depth = depth_dev; x.length = length_dev; x.keys = keys_dev; x.masks = masks_dev; x.count = count; x.stride = stride; x.n = n_steps;
    return grow(h, t, x);
}

int ngw_tree_backup(ngw_handle* h, ngw_tree* t, const int32_t* actions_dev, const int32_t* rewards_dev, const int32_t* where_dev, const int32_t* depth_dev,
                    const int32_t* length_dev, int64_t stride, int64_t count, int32_t n_steps, int32_t use_leaves, const int32_t* bootstrap_dev) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (int rc = stage_args(t, stride, count, n_steps)) return rc;
    if (count && (!actions_dev || !rewards_dev || !where_dev || !depth_dev || !length_dev)) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    NgwTree x = tree_args(h, t);
    x.actions = actions_dev; x.rewards = rewards_dev; x.where = where_dev; x.depth = depth_dev; x.length = length_dev; x.bootstrap = bootstrap_dev;
    x.count = count; x.stride = stride; x.n = n_steps;
    if (!use_leaves) x.where_leaf = nullptr;
    return backup(h, t, x);
}

int ngw_tree_reweight(ngw_handle* h, ngw_tree* t, const int32_t* buckets_dev, int64_t count) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (count < 0 || count > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "a list of %lld buckets", (long long)count);
    if (int rc = enter(h)) return rc;
    const NgwTree x = tree_args(h, t);
    if (!buckets_dev) return reweight(h, t, x, t->touched, (int64_t)t->T * t->cap);
    return reweight(h, t, x, buckets_dev, count);
}

int ngw_tree_set_rule(ngw_handle* h, ngw_tree* t, const ngw_tree_rule* rule) {
    if (!h || !t || !rule) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = tree_call_args(h, t)) return rc;
    if (rule->spread < 1 || rule->spread > 64) return fail(NGW_E_INVALID_ARG, "tree rule: spread = %d outside [1, 64]", (int)rule->spread);
    if (rule->discount_q16 < 0 || rule->discount_q16 > 65536) return fail(NGW_E_INVALID_ARG, "tree rule: discount_q16 = %d outside [0, 65536]", (int)rule->discount_q16);
    if (rule->rows16 < 0 || rule->rows16 > 2) return fail(NGW_E_INVALID_ARG, "tree rule: rows16 = %d outside [0, 2]", (int)rule->rows16);
    if (rule->rows16 == 2 && rule->spread > 1) return fail(NGW_E_INVALID_ARG, "tree rule: rows16 = 2 (the one-lane reweight) serves spread = 1 only, not %d", (int)rule->spread);
    if (rule->reserved != 0) return fail(NGW_E_INVALID_ARG, "tree rule: reserved = %d, 0 expected", (int)rule->reserved);
    if (int rc = enter(h)) return rc;
    // the list of the last backup is forgotten, in stream order: ngw_tree_reweight(NULL) never rewrites rows under a rule their backup did not run under
    HIP_TRY(hipMemsetAsync(t->touched, 0xFF, (size_t)t->T * (size_t)t->cap * 4, h->stream));
    t->spread = rule->spread; t->discount_q16 = rule->discount_q16; t->rows16 = rule->rows16;   // (host state, read by the calls enqueued from here on)
    return NGW_OK;
}

int ngw_tree_report(ngw_handle* h, ngw_tree* t, ngw_tree_report_rows* out) {
    if (!h || !t || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->trees, t)) return fail(NGW_E_INVALID_ARG, "not an open tree search of this handle");
    if (int rc = enter(h)) return rc;
    uint32_t ring[TREE_RING][NGW_TREE_COLS];
    uint32_t flags = 0;
    HIP_TRY(hipMemcpyAsync(ring, t->stats, sizeof(ring), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(&flags, h->b.flags, sizeof(flags), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->b.flags_host) flags |= *h->b.flags_host;
    memset(out, 0, sizeof(*out));
    out->iterations = t->iterations;
    out->flags = flags;
    out->rows = (int32_t)(t->iterations < NGW_TREE_ROWS ? t->iterations : NGW_TREE_ROWS);
    for (int32_t i = 0; i < out->rows; i++)
        memcpy(out->stats[i], ring[(t->iterations - (uint64_t)out->rows + (uint64_t)i) % TREE_RING], sizeof(out->stats[0]));
    return NGW_OK;
}

int ngw_tree_clear(ngw_handle* h, ngw_tree* t) {
    if (int rc = tree_call_args(h, t)) return rc;
    if (int rc = enter(h)) return rc;
    if (int rc = ngw_key_table_clear(h, t->table)) return rc;
    return zero_statistics(h, t);
}

}  // extern "C"
