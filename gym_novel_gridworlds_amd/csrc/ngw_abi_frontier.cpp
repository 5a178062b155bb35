// ngw_abi_frontier.cpp - device-side frontiers (see ngw_host.h): a flag array compacted into an index list of fixed capacity, padded with
// NGW_IDX_NONE, and slots handed out for it from a cursor in device memory (ngw_frontier.inc); the `keep` best candidates of every group of values
// in the same list form (ngw_select.inc).  The calls write no env state: they neither call state_written() nor touch anything the handle derives
// from its state.  All run on the handle's stream, behind enter(), and wait for nothing.
#include "ngw_host.h"

using namespace ngwh;

namespace {

// the handle's scratch with room for `tiles` tile counts behind the ticket word (zero-filled on the handle's stream when it is allocated)
int frontier_scratch(ngw_handle* h, int64_t tiles) {
    if (h->frontier_scratch && tiles <= h->frontier_tiles) return NGW_OK;
    if (h->frontier_scratch) {
        HIP_TRY(hipStreamSynchronize(h->stream));                                  // (a compaction may still be using the old one)
        dev_free(h, h->frontier_scratch);
        h->frontier_scratch = nullptr;
        h->frontier_tiles = 0;
    }
    const int64_t room = tiles < 512 ? 512 : tiles;                               // (512 tiles: 2^21 flags)
    if (int rc = dev_alloc(h, &h->frontier_scratch, (size_t)room + 1)) return rc;
    h->frontier_tiles = room;
    return NGW_OK;
}

// the handle's scratch of ngw_frontier_select with room for `words` words (zero-filled on the handle's stream when it is allocated: the wave
// form's ticket word is 0 between the calls; the grid form zero-fills what it uses in every call)
int select_scratch(ngw_handle* h, int64_t words) {
    if (h->select_scratch && words <= h->select_words) return NGW_OK;
    if (h->select_scratch) {
        HIP_TRY(hipStreamSynchronize(h->stream));                                  // (a selection may still be using the old one)
        dev_free(h, h->select_scratch);
        h->select_scratch = nullptr;
        h->select_words = 0;
    }
    const int64_t room = words < 4096 ? 4096 : words;
    if (int rc = dev_alloc(h, &h->select_scratch, (size_t)room)) return rc;
    h->select_words = room;
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_frontier_compact(ngw_handle* h, const uint8_t* flags_dev, int64_t n, int32_t div, const int32_t* map_dev, int64_t capacity, int32_t* first_dev,
                         int32_t* second_dev, int32_t* count_dev) {
    if (!h || !count_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (n < 0 || n > NGW_FRONTIER_MAX_FLAGS) return fail(NGW_E_INVALID_ARG, "compaction of %lld flags (at most %lld)", (long long)n, (long long)NGW_FRONTIER_MAX_FLAGS);
    if (n && !flags_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (div < 1) return fail(NGW_E_INVALID_ARG, "compaction with div %d: at least 1 expected", (int)div);
    if (capacity < 0 || capacity > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "frontier capacity %lld", (long long)capacity);
    if (capacity && !first_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    const int64_t tiles = (n + NGW_FRONTIER_TILE - 1) / NGW_FRONTIER_TILE;
    if (int rc = frontier_scratch(h, tiles)) return rc;
    NgwFrontier x{};
    x.bytes = flags_dev; x.map = map_dev; x.first = first_dev; x.second = second_dev; x.count = count_dev;
    x.tiles = h->frontier_scratch + 1; x.flags = h->b.flags;
    x.n = n; x.capacity = capacity; x.div = div; x.n_tiles = (int32_t)tiles;
    HIP_TRY(ngw_frontier_compact_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_frontier_alloc(ngw_handle* h, const int32_t* count_dev, int32_t* cursor_dev, int32_t limit, int64_t capacity, int32_t* slots_dev) {
    if (!h || !count_dev || !cursor_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (limit < 0) return fail(NGW_E_INVALID_ARG, "slot limit %d", (int)limit);
    if (capacity < 0 || capacity > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "frontier capacity %lld", (long long)capacity);
    if (capacity && !slots_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    if (int rc = frontier_scratch(h, 0)) return rc;
    NgwFrontierAlloc x{};
    x.count = count_dev; x.cursor = cursor_dev; x.slots = slots_dev; x.ticket = reinterpret_cast<uint32_t*>(h->frontier_scratch); x.flags = h->b.flags;
    x.capacity = capacity; x.limit = limit;
    HIP_TRY(ngw_frontier_alloc_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_frontier_select(ngw_handle* h, const int32_t* values_dev, const uint8_t* flags_dev, int64_t n, int32_t groups, int32_t div, const int32_t* map_dev,
                        int32_t keep, int32_t largest, int64_t capacity, int32_t* first_dev, int32_t* second_dev, int32_t* taken_dev, int32_t* bound_dev,
                        int32_t* count_dev) {
    if (!h || !count_dev || !taken_dev || !bound_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (n < 0 || n > NGW_SELECT_MAX_VALUES) return fail(NGW_E_INVALID_ARG, "selection among %lld values (at most %lld)", (long long)n, (long long)NGW_SELECT_MAX_VALUES);
    if (groups < 1 || groups > NGW_SELECT_MAX_VALUES || n % groups) return fail(NGW_E_INVALID_ARG, "selection of %lld values in %d groups", (long long)n, (int)groups);
    if (n && !values_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (div < 1) return fail(NGW_E_INVALID_ARG, "selection with div %d: at least 1 expected", (int)div);
    if (keep < 0) return fail(NGW_E_INVALID_ARG, "selection of %d per group", (int)keep);
    if (largest != 0 && largest != 1) return fail(NGW_E_INVALID_ARG, "largest %d: 0 or 1 expected", (int)largest);
    if (capacity < 0 || capacity > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "frontier capacity %lld", (long long)capacity);
    if ((int64_t)groups * keep > capacity) return fail(NGW_E_INVALID_ARG, "%d groups of %d entries in a list of %lld", (int)groups, (int)keep, (long long)capacity);
    if (capacity && !first_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter(h)) return rc;
    const int64_t m = n / groups, tpg = (m + NGW_FRONTIER_TILE - 1) / NGW_FRONTIER_TILE;
    if (int rc = select_scratch(h, m <= NGW_SELECT_WAVE_MAX ? 2 : NGW_SELECT_SCRATCH_WORDS(groups, tpg))) return rc;
    NgwSelect x{};
    x.values = values_dev; x.bytes = flags_dev; x.map = map_dev; x.first = first_dev; x.second = second_dev; x.taken = taken_dev; x.bound = bound_dev;
    x.count = count_dev; x.scratch = h->select_scratch;
    x.capacity = capacity; x.groups = groups; x.m = (int32_t)m; x.div = div; x.keep = keep; x.largest = largest; x.tiles_per_group = (int32_t)tpg;
    HIP_TRY(ngw_frontier_select_launch(&x, h->stream));
    return NGW_OK;
}

}  // extern "C"
