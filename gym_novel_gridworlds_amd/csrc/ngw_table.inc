// ngw_table.inc - the device-side key table (a unit of its own; host side: ngw_abi_table.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// An open-addressing set of 64-bit keys: "have I seen this state before?" for a search that runs many iterations.  Storage is two arrays of
// `buckets` (a power of two) 64-bit words: key[] (0 = empty) and stamp[] (all ones = nobody has offered this bucket's key yet), and one counter.
//
// Insert, launch 1 (table_probe<true>): one lane per key.  The start bucket is the splitmix64 finaliser of the key (callers' keys need not have
// good low bits), then linear probing: a relaxed agent-scope load of the bucket; an empty one is claimed with a 64-bit compare-and-swap 0 -> key,
// and a swap that loses to another lane is read as what the winner wrote (the same key: found; another: go on).  Buckets only ever go from empty
// to occupied, so two lanes that carry one key walk the same occupied prefix and meet in the same bucket: a key is stored once.  A lane that
// found or placed its key writes where[j] and lowers stamp[bucket] to base + j with a 64-bit atomic min.  A lane that has looked at EVERY bucket
// and found neither its key nor room gives up (where = -1, NGW_F_TABLE_FULL): every bucket was occupied when it looked, so the table is full.
// Nothing waits for another lane: 64 lanes that fight for one bucket each do one swap and go on.
// Insert, launch 2 (table_fresh): fresh[j] = (stamp[where[j]] == base + j).  `base` (the host's running total of keys ever offered) only grows,
// so a key stored by an earlier call holds a smaller stamp than any position of this call, and among the positions of this call that carry a
// new key the smallest wins whatever order the lanes ran in: `fresh` is deterministic where the choice of the bucket is not.
// The two launches are not folded into one: position j may only be called fresh once EVERY lane of the call that carries the same key has made
// its atomic min, which one launch could only know by waiting for other work-groups.
// Lookup (table_probe<false>): the same walk with plain loads; it ends at the key or at an empty bucket.  The walk is table_find below - the
// one statement of the read-only probe, which the guided playout (ngw_playout.inc, GUIDED) calls for the state a pair is in at every step.
// No early exit: every lane reaches the wave-wide count of placed keys (one atomic add per wave).
// The kernels are the table unit's alone (ngw_unit_table.hip defines NGW_TABLE_UNIT); every other unit that includes this file gets the walk.

__device__ __forceinline__ uint64_t table_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The read-only walk: the bucket of `key[]` (mask + 1 of them, a power of two) that holds `key` (never 0: the caller answers -1 for it), or -1
// where the walk meets an empty bucket or has looked at every bucket.  Plain loads, no store, no wait for another lane; it diverges per lane
// and is bounded by the number of buckets.  Every address is b & mask: inside the table whatever the key.
__device__ __forceinline__ int32_t table_find(const uint64_t* __restrict__ keys, uint64_t mask, uint64_t key) {
    uint64_t b = table_mix64(key) & mask;
    for (uint64_t n = 0; n <= mask; n++, b = (b + 1) & mask) {
        const uint64_t cur = keys[b];
        if (!cur) break;                                           // absent
        if (cur == key) return (int32_t)b;
    }
    return -1;
}

#ifdef NGW_TABLE_UNIT
template <bool INSERT>
__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_probe_kernel(const NgwTable x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    const bool inside = j < x.count;
    const uint64_t key = inside ? x.keys[j] : 0ull;               // (key 0 is never stored: the empty mark, and ngw_state_keys' answer to a bad index)
    int32_t where = -1;
    bool placed = false, refused = false;
    if constexpr (!INSERT) {
        if (key) where = table_find(x.key, x.mask, key);
    } else if (key) {
        uint64_t b = table_mix64(key) & x.mask;
        refused = true;
        for (uint64_t n = 0; n <= x.mask; n++, b = (b + 1) & x.mask) {
            uint64_t cur = __hip_atomic_load(x.key + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!cur) {
                if (__hip_atomic_compare_exchange_strong(x.key + b, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    placed = true;
                    cur = key;
                }                                                  // (a lost swap left the winner's key in `cur`)
            }
            if (cur == key) { where = (int32_t)b; refused = false; break; }
        }
        if (where >= 0) __hip_atomic_fetch_min(x.stamp + where, x.base + (uint64_t)j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (inside) x.where[j] = where;
    if (INSERT) {
        const uint32_t n_placed = (uint32_t)__popcll(__ballot(placed));
        if ((threadIdx.x & (EPB - 1)) == 0 && n_placed) atomicAdd(x.stored, (unsigned long long)n_placed);
        if (refused) atomicOr(x.flags, NGW_F_TABLE_FULL);
    }
}

__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_fresh_kernel(const NgwTable x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    if (j >= x.count) return;
    const int32_t w = x.where[j];
    x.fresh[j] = ((uint64_t)(int64_t)w <= x.mask && x.stamp[w] == x.base + (uint64_t)j) ? 1 : 0;
}
#endif  // NGW_TABLE_UNIT

}  // namespace
