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

// The walk heuristic of one row of K distances (ngw_device.h): K consecutive int32 beside the K weights, read as 16-byte, 8-byte or 4-byte words -
// whichever K lets every row start on (both arrays start on 16 bytes).  Integer arithmetic: the product in 64 bits, clamped.
__device__ __forceinline__ void search_h_term(int32_t w, int32_t d, int32_t mode, int64_t& acc, bool& any) {
    if (w > 0 && d >= 0) {
        const int64_t t = (int64_t)w * (int64_t)d;
        acc = !any ? t : (mode == NGW_SEARCH_H_MAX ? (t > acc ? t : acc) : (t < acc ? t : acc));
        any = true;
    }
}

__device__ __forceinline__ int32_t search_walk_h(const int32_t* __restrict__ d, const int32_t* __restrict__ w, int32_t K, int32_t mode) {
    int64_t acc = 0;
    bool any = false;
    if ((K & 3) == 0) {
        for (int32_t k = 0; k < K; k += 4) {
            const int4 dd = *reinterpret_cast<const int4*>(d + k), ww = *reinterpret_cast<const int4*>(w + k);
            search_h_term(ww.x, dd.x, mode, acc, any); search_h_term(ww.y, dd.y, mode, acc, any);
            search_h_term(ww.z, dd.z, mode, acc, any); search_h_term(ww.w, dd.w, mode, acc, any);
        }
    } else if ((K & 1) == 0) {
        for (int32_t k = 0; k < K; k += 2) {
            const int2 dd = *reinterpret_cast<const int2*>(d + k), ww = *reinterpret_cast<const int2*>(w + k);
            search_h_term(ww.x, dd.x, mode, acc, any); search_h_term(ww.y, dd.y, mode, acc, any);
        }
    } else {
        for (int32_t k = 0; k < K; k++) search_h_term(w[k], d[k], mode, acc, any);
    }
    const int64_t top = (int64_t)NGW_VALUE_NONE - 1;
    return (int32_t)(acc > top ? top : acc);
}

// f of a slot reached with g under the heuristic h: the sum in 64 bits, below NGW_VALUE_NONE so that it stays a candidate of the selection
__device__ __forceinline__ int32_t search_priority(int32_t g, int32_t h) {
    const int64_t sum = (int64_t)g + (int64_t)h, top = (int64_t)NGW_VALUE_NONE - 1;
    return (int32_t)(sum > top ? top : sum);
}

// OPEN: the superseding of step 6 and the reset of the open-list stats row.  The closed instantiation is the kernel as it was.
template <bool OPEN>
__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_settle_kernel(const NgwSearch x) {
    const int64_t k = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    bool live = false, superseded = false;
    if (k < x.capacity) {
        const int32_t j = x.first[k], a = x.second[k], c = x.slots[k];
        const bool entry = j >= 0 && (int64_t)j < x.capacity && a >= 0 && a < x.A;
        live = entry && c >= 0 && (int64_t)c < x.pool;
        x.plist[k] = entry ? x.parents[j] : NGW_IDX_NONE;
        if (live) {
            const int64_t q = (int64_t)j * x.A + a;
            x.g[c] = x.values[q];
            x.bucket[c] = x.where[q];
            if constexpr (OPEN) {
                const int32_t b = x.where[q];
                if (b >= 0 && (int64_t)b < x.buckets) {
                    // insert_min sets best at most once per key and call, and a bucket holds one key: this lane is the only one of the iteration
                    // that reads or writes slot_of_bucket[b], and - a slot has one bucket - the only one that closes `old`.  No atomic is needed.
                    const int32_t old = x.slot_of_bucket[b];
                    superseded = old >= 0 && (int64_t)old < x.pool && old != c;
                    if (superseded) x.f[old] = NGW_VALUE_NONE;                     // reached more cheaply: never expanded from the dearer copy
                    x.slot_of_bucket[b] = c;
                }
            }
        }
        x.next[k] = live ? c : NGW_IDX_NONE;
    }
    const uint32_t count = search_wave_count(live);
    if (search_wave_leader() && count) atomicAdd(x.row + NGW_SEARCH_EXPANDED, count);
    if constexpr (OPEN) {
        const uint32_t closed = search_wave_count(superseded);
        if (search_wave_leader() && closed) atomicAdd(x.orow + NGW_SEARCH_SUPERSEDED, closed);
    }
    if (k == 0) {
        for (int i = 0; i < 4; i++) x.next_row[i] = 0;
        if constexpr (OPEN) {
            for (int i = 0; i < NGW_SEARCH_OPEN_COLS; i++) x.next_orow[i] = 0;
            x.next_orow[NGW_SEARCH_FMIN] = (uint32_t)NGW_VALUE_NONE;
            x.next_orow[NGW_SEARCH_FBOUND] = (uint32_t)INT32_MIN;
        }
    }
}

// TAKE (step 0): the chosen slots are closed; with prune, those that cannot beat the goal are taken off the parent list
__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_take_kernel(const NgwSearch x) {
    const int64_t k = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    bool chosen = false, pruned = false;
    int32_t lo = NGW_VALUE_NONE, hi = INT32_MIN;
    if (k < x.capacity) {
        int32_t* const P = const_cast<int32_t*>(x.parents);
        const int32_t slot = P[k];
        chosen = slot >= 0 && (int64_t)slot < x.pool;
        if (chosen) {
            const int32_t old = x.f[slot];
            x.f[slot] = NGW_VALUE_NONE;
            lo = hi = old;
            if (x.prune) {
                const int32_t goal = (int32_t)((uint32_t)(*x.goal >> 32) ^ 0x80000000u);   // (no goal yet: all ones, NGW_VALUE_NONE - above every f)
                pruned = old >= goal;
                if (pruned) P[k] = NGW_IDX_NONE;
            }
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const int32_t a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const uint32_t n_chosen = search_wave_count(chosen), n_pruned = search_wave_count(pruned);
    if (search_wave_leader() && n_chosen) {
        atomicAdd(x.orow + NGW_SEARCH_CHOSEN, n_chosen);
        if (n_pruned) atomicAdd(x.orow + NGW_SEARCH_PRUNED, n_pruned);
        atomicMin(reinterpret_cast<int32_t*>(x.orow) + NGW_SEARCH_FMIN, lo);
        atomicMax(reinterpret_cast<int32_t*>(x.orow) + NGW_SEARCH_FBOUND, hi);
    }
    if (k == 0) x.orow[NGW_SEARCH_OPEN] = (uint32_t)x.sel_count[1];
}

// OPEN (step 8): h and f of every child written this iteration; h = the walk term plus, where the search has one, the recipe term, clamped
__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_open_kernel(const NgwSearch x) {
    const int64_t k = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    if (k >= x.capacity) return;
    const int32_t c = x.next[k];
    if (c < 0 || (int64_t)c >= x.pool) return;
    int32_t hv = x.dist ? search_walk_h(x.dist + k * x.K, x.weights, x.K, x.mode) : 0;
    if (x.recipe) hv = search_priority(hv, x.recipe[k]);                               // (the two terms add: movement and rule actions are disjoint)
    x.h[c] = hv;
    x.f[c] = search_priority(x.g[c], hv);
}

template <bool OPEN>
__global__ void __launch_bounds__(NGW_SEARCH_BLOCK) ngw_search_roots_kernel(const NgwSearchRoots x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_SEARCH_BLOCK + threadIdx.x;
    if (j >= x.capacity) return;
    int32_t parent = NGW_IDX_NONE;
    if (j < x.count) {
        const int32_t r = x.roots[j], w = x.where[j];
        if (r >= 0 && (int64_t)r < x.pool && w >= 0) {
            const int32_t g = x.value[j];
            x.g[r] = g;
            x.bucket[r] = w;
            if (x.best[j]) {
                if constexpr (OPEN) {                                              // opened: the first iteration chooses it from the list
                    if ((int64_t)w < x.buckets) x.slot_of_bucket[w] = r;           // (best is set once per key: one writer per bucket)
                    int32_t hv = x.dist ? search_walk_h(x.dist + j * x.K, x.weights, x.K, x.mode) : 0;
                    if (x.recipe) hv = search_priority(hv, x.recipe[j]);
                    x.h[r] = hv;
                    x.f[r] = search_priority(g, hv);
                } else {
                    parent = r;
                }
            }
        }
    }
    x.parents[j] = parent;
}

}  // namespace
