// ngw_table.inc - the device-side key table (a unit of its own; host side: ngw_abi_table.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// An open-addressing set of 64-bit keys: "have I seen this state before?" for a search that runs many iterations.  Storage is two arrays of
// `buckets` (a power of two) 64-bit words: key[] (0 = empty) and stamp[] (all ones = nobody has offered this bucket's key yet), and one counter.
// A VALUED table (ngw_key_table_create_valued) holds two more arrays behind them: best[] (one 64-bit word per bucket, below) and tag[] (one
// int32 per bucket, -1 = NGW_TAG_ROOT until a tag is stored); a table without values has neither and runs exactly the launches it always ran.
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
//
// insert_min (table_probe<true, true> and table_fresh<true>) is the same two launches with one more atomic min beside the one on the stamp.
// best[b] = (uint32(value) ^ 0x80000000) << 32 | seq32: the bucket's value, biased so that the unsigned order of the word is the signed order
// of the value, above the low half of the base + j that offered it.  All ones = never valued: NGW_VALUE_NONE biased is the largest high half,
// and a position whose value is NGW_VALUE_NONE makes no offer, so no offer ever equals the mark.  Launch 1 lowers best[where[j]] to position
// j's word; launch 2 sets improved[j] = (best[where[j]] == my word), and that one lane per bucket stores its tag.  A smaller value wins by the
// high half; among equal values of one call the smaller position wins by the low half; an equal value of a LATER call carries a larger seq32
// than the word in the table and changes nothing - the strict comparison of the contract.  That needs seq32 to grow from call to call, so
// before a call whose positions would carry the low half past 2^32 the host enqueues table_renorm - every valued word's low half to 0 - and
// moves `base` up to the next multiple of 2^32 plus one (the stamps only ask that base grows): once per 2^32 keys offered, a pass over the
// buckets; every other call costs what its batch costs.  No lane waits for another, and there is no reset pass between the calls.
// read (table_read): value and tag by bucket, one lane per query.  trace (table_trace): one lane per query follows tag = parent_bucket * A +
// action from a bucket to its root, at most T links - tags are the caller's data and may form cycles -, once to count and once more to write
// the actions in execution order; every tag is checked against [0, buckets * A) before it becomes an address.
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
// position j's word of an insert_min: the biased value above the low half of base + j
__device__ __forceinline__ uint64_t table_word(int32_t value, uint64_t base, int64_t j) {
    return ((uint64_t)((uint32_t)value ^ 0x80000000u) << 32) | (uint64_t)(uint32_t)(base + (uint64_t)j);
}

template <bool INSERT, bool VALUED = false>
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
        if constexpr (VALUED) {
            if (where >= 0) {
                const int32_t v = x.values[j];
                if (v != NGW_VALUE_NONE) __hip_atomic_fetch_min(x.best + where, table_word(v, x.base, j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (inside) x.where[j] = where;
    if (INSERT) {
        const uint32_t n_placed = (uint32_t)__popcll(__ballot(placed));
        if ((threadIdx.x & (EPB - 1)) == 0 && n_placed) atomicAdd(x.stored, (unsigned long long)n_placed);
        if (refused) atomicOr(x.flags, NGW_F_TABLE_FULL);
    }
}

template <bool VALUED = false>
__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_fresh_kernel(const NgwTable x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    if (j >= x.count) return;
    const int32_t w = x.where[j];
    const bool held = (uint64_t)(int64_t)w <= x.mask;
    x.fresh[j] = (held && x.stamp[w] == x.base + (uint64_t)j) ? 1 : 0;
    if constexpr (VALUED) {
        const int32_t v = x.values[j];
        const bool won = held && v != NGW_VALUE_NONE && x.best[w] == table_word(v, x.base, j);
        x.improved[j] = won ? 1 : 0;
        if (won && x.tags) x.tag[w] = x.tags[j];                  // (one winner per bucket and call: a plain store)
    }
}

// every valued word's low half to 0 (a never-valued word stays all ones): the sequence starts again above it
__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_renorm_kernel(uint64_t* __restrict__ best, uint64_t buckets) {
    const uint64_t b = (uint64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    if (b >= buckets) return;
    const uint64_t w = best[b];
    if (w != ~0ull) best[b] = w & 0xFFFFFFFF00000000ull;
}

__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_read_kernel(const NgwTableRead x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    if (j >= x.count) return;
    const int32_t w = x.where[j];
    int32_t value = NGW_VALUE_NONE, tag = NGW_TAG_ROOT;
    if ((uint64_t)(int64_t)w <= x.mask) {
        value = (int32_t)((uint32_t)(x.best[w] >> 32) ^ 0x80000000u);
        tag = x.tag[w];
    } else if (w != -1 && w != NGW_IDX_NONE) {
        atomicOr(x.flags, NGW_F_BAD_INDEX);
    }
    x.value[j] = value;
    x.tag_out[j] = tag;
}

// One link of a trace from bucket b: 0 - b holds a root; 1 - *up is the parent's bucket and *act the action; 2 - a bucket outside the table,
// an empty one, or a tag outside [0, buckets * A); 3 - no root, and `follow` is off: the chain is longer than the caller follows (its next
// tag is not looked at).  b is checked before it is an address, and so is every bucket a tag names.
__device__ __forceinline__ int table_link(const NgwTableTrace& x, int64_t b, bool follow, int64_t* up, int32_t* act) {
    if ((uint64_t)b > x.mask || !x.key[b]) return 2;
    const int32_t tg = x.tag[b];
    if (tg == NGW_TAG_ROOT) return 0;
    if (!follow) return 3;
    if (tg < 0 || (int64_t)tg >= (int64_t)(x.mask + 1) * x.A) return 2;
    *up = tg / x.A;
    *act = tg % x.A;
    return 1;
}

__global__ void __launch_bounds__(NGW_TABLE_BLOCK) ngw_table_trace_kernel(const NgwTableTrace x) {
    const int64_t j = (int64_t)blockIdx.x * NGW_TABLE_BLOCK + threadIdx.x;
    if (j >= x.count) return;
    const int32_t w = x.where[j];
    int32_t length = -1, root = -1;
    bool bad = false;
    if (w != -1 && w != NGW_IDX_NONE) {
        int64_t b = w, up = 0;
        int32_t act = 0;
        for (int32_t n = 0; n <= x.T; n++) {                       // (T links at most: the T + 1-th look only asks whether link T ended in a root)
            const int r = table_link(x, b, n < x.T, &up, &act);
            if (r == 0) { length = n; root = (int32_t)b; break; }
            if (r == 2) { bad = true; break; }
            if (r == 3) break;
            b = up;
        }
    }
    if (bad) atomicOr(x.flags, NGW_F_BAD_INDEX);
    x.length[j] = length;
    x.root[j] = root;
    for (int32_t t = length < 0 ? 0 : length; t < x.T; t++) x.plans[(int64_t)t * x.count + j] = -1;
    int64_t b = w, up = 0;
    for (int32_t n = length - 1; n >= 0; n--) {                    // (the links the first walk has checked, now from the last move to the first)
        int32_t act = 0;
        table_link(x, b, true, &up, &act);
        x.plans[(int64_t)n * x.count + j] = act;
        b = up;
    }
}
#endif  // NGW_TABLE_UNIT

}  // namespace
