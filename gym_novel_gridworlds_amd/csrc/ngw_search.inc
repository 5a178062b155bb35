// ngw_search.inc - search runs: the glue of one best-first iteration between successor keys, insert_min, compaction / selection, slot allocation
// and expand, on the device (a unit of its own; host side: ngw_abi_search.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// The loop of key_table.py's docstring is six library calls and, between them, torch operations that gather each parent's cost and bucket, add the
// step costs, build the tags and - behind the expand - look every child up again to learn what the call before already knew.  Here that glue is
// three kernels (NgwSearch in ngw_device.h says what each stores; the contract is include/ngw.h's ngw_search_run, search.relax_reference states it in
// numpy), so that a driver on the host can enqueue whole iterations without a torch operation in between.
//
// All three give one position - or one list entry - to a lane: consecutive lanes read and write consecutive int32 / uint32 words (the parents' g and
// bucket are gathers: A consecutive lanes share one parent, so a wave touches 64 / A + 1 of them), no LDS, no float, vector memory operations only.
// What is counted or minimised over the positions is reduced inside the wave first - a ballot for the counts, six xor shuffles for the goal word -
// and reaches memory as at most one atomic per wave and quantity.  The goal word orders (value, bucket) pairs as one uint64: the value with its sign
// bit flipped in the high half (the table's own order of values, ngw_table.inc), the bucket below; a bucket holds one key, so the smallest pair
// does not depend on the order the waves arrive in.

constexpr unsigned long long SEARCH_NO_GOAL = ~0ull;

// the lanes of the wave for which `p` holds, counted once: lane 0's to add
__device__ __forceinline__ uint32_t search_wave_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__device__ __forceinline__ bool search_wave_leader() { return (threadIdx.x & (EPB - 1)) == 0; }

__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_offer_kernel(const NgwSearch x) {
    const int64_t q = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x, n = x.capacity * x.A;
    const bool in = q < n;
    int32_t value = NGW_VALUE_NONE, tag = NGW_TAG_ROOT;
    bool over = false;
    if (in) {
        const int32_t j = (int32_t)(q / x.A), a = (int32_t)(q - (int64_t)j * x.A);
        const int32_t p = x.parents[j];
        const uint32_t w = x.info[q];
        if (p >= 0 && (int64_t)p < x.pool) {                                       // (NGW_IDX_NONE is negative: a padded parent offers nothing)
            const int32_t gp = x.g[p];
            if (gp != NGW_VALUE_NONE) {
                const int64_t sum = (int64_t)gp + (int64_t)x.lut[x.by_action ? (uint32_t)a : NGW_INFO_COST(w)];
                over = sum >= (int64_t)NGW_VALUE_NONE || sum < (int64_t)INT32_MIN;
                if (!over) {
                    value = (int32_t)sum;
                    tag = x.bucket[p] * x.A + a;
                }
            }
        }
        x.values[q] = value;
        x.tags[q] = tag;
    }
    const uint32_t offers = search_wave_count(value != NGW_VALUE_NONE), overs = search_wave_count(over);
    if (search_wave_leader()) {
        if (offers) atomicAdd(x.row + NGW_SEARCH_OFFERED, offers);
        if (overs) {
            atomicAdd(x.row + NGW_SEARCH_OVERFLOW, overs);
            atomicAdd(x.overflowed, (unsigned long long)overs);
        }
    }
}

__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_judge_kernel(const NgwSearch x) {
    const int64_t q = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x, n = x.capacity * x.A;
    bool improved = false;
    unsigned long long word = SEARCH_NO_GOAL;
    if (q < n) {
        improved = x.best[q] != 0;
        const uint32_t w = x.info[q];
        const bool ended = NGW_INFO_DONE(w) != 0;
        if (improved && ended && NGW_INFO_MSG(w) != 14u)                           // (message code 14: a FireWall death, no goal - Expansion.goal / .died)
            word = (unsigned long long)((uint32_t)x.values[q] ^ 0x80000000u) << 32 | (uint32_t)x.where[q];
        if (x.stop && ended && improved) x.best[q] = 0;                            // (an ended state is stored and valued, never expanded)
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long other = __shfl_xor(word, off);
        word = other < word ? other : word;
    }
    const uint32_t count = search_wave_count(improved);
    if (search_wave_leader()) {
        if (count) atomicAdd(x.row + NGW_SEARCH_IMPROVED, count);
        if (word != SEARCH_NO_GOAL) atomicMin(x.goal, word);
    }
}

__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_settle_kernel(const NgwSearch x) {
    const int64_t k = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    bool live = false;
    if (k < x.capacity) {
        const int32_t j = x.first[k], a = x.second[k], c = x.slots[k];
        const bool entry = j >= 0 && (int64_t)j < x.capacity && a >= 0 && a < x.A;
        live = entry && c >= 0 && (int64_t)c < x.pool;
        x.plist[k] = entry ? x.parents[j] : NGW_IDX_NONE;
        if (live) {
            const int64_t q = (int64_t)j * x.A + a;
            x.g[c] = x.values[q];
            x.bucket[c] = x.where[q];
        }
        x.next[k] = live ? c : NGW_IDX_NONE;
    }
    const uint32_t count = search_wave_count(live);
    if (search_wave_leader() && count) atomicAdd(x.row + NGW_SEARCH_EXPANDED, count);
    if (k == 0)
        for (int i = 0; i < 4; i++) x.next_row[i] = 0;
}

__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_roots_kernel(const NgwSearchRoots x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    if (j >= x.capacity) return;
    int32_t parent = NGW_IDX_NONE;
    if (j < x.count) {
        const int32_t r = x.roots[j], w = x.where[j];
        if (r >= 0 && (int64_t)r < x.pool && w >= 0) {
            x.g[r] = x.value[j];
            x.bucket[r] = w;
            if (x.best[j]) parent = r;
        }
    }
    x.parents[j] = parent;
}

}  // namespace
