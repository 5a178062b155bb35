// ngw_keys.inc - device-side state keys (a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// keys[j] = the 64-bit key of row idx[j] of a set of state rows (a snapshot, or the state slab) under the field selection `fields`.  The key is
// a public contract (include/ngw.h, ngw_state_keys): the XOR of independent terms
//     term(tag, index, value) = mix64((uint64)tag << 56 | (uint64)index << 32 | (uint32)value)          (mix64: the splitmix64 finaliser)
// one per non-zero group of four map cells, one for the pose, one per non-zero inventory entry, one each for the selected item, the step count
// and the episode counter.  XOR commutes, so which lane hashes which term, and in which order they meet, does not show in the result.
//
// Shape: the snapshot copy's reads under the lidar slot kernel's decomposition, and no LDS.  One work-group is one wave: 64 consecutive pairs.
//   1. Lane l reads idx[l] (NULL: l), compares it with the row count as an unsigned number and clamps a bad one to row 0 - nothing is ever
//      addressed with the bad index; its key is 0 and NGW_F_BAD_INDEX is raised.  The lane gathers its row's five scalars and hashes their terms:
//      every lane busy once, where a lane of each round's group would do it sixteen times over with 60 lanes idle.
//   2. Sixteen rounds of four rows: NGW_SNAP_GROUP = 16 lanes share one row, consecutive lanes load consecutive 16-byte pieces (S*S a multiple
//      of 16), dwords (a multiple of 4) or - odd S*S - dwords at whatever byte address the row starts (global memory takes them) and the
//      one-cell tail as a byte; then the inventory dwords.  Everything goes from HBM into registers and is read once.  Group q = lane / 16 takes
//      row 16 * q + r in round r, its index out of the owner's register with ds_bpermute: the owner is lane r OF THE SAME GROUP, so after the
//      reduction the key is where it is stored from and no value crosses a group.
//   3. Each lane hashes the groups of its own pieces; the 16 lanes XOR-reduce the two 32-bit halves inside the DPP row with row_ror 8 / 4 / 2 / 1
//      (a rotation, so every lane ends with the whole XOR; gfx9 has no row_xmask).  Lane r of the group keeps it.
//   4. Lane l holds key l: one coalesced 512-byte store per wave, bounded by count.
// No early exit: every lane is active at every DPP step and every ds_bpermute.

__device__ __forceinline__ uint64_t key_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// (tag and index share the head's 32 bits: an index - a map group or an item - stays below 2^24)
static_assert(NGW_MAX_MAP_SIZE * NGW_MAX_MAP_SIZE / 4 < (1 << 24) && NGW_MAX_ITEMS < (1 << 24), "key_term packs tag << 24 | index");
__device__ __forceinline__ uint64_t key_term(uint32_t tag, uint32_t index, uint32_t value) {
    return key_mix64((uint64_t)(tag << 24 | index) << 32 | value);
}
// the term of map group `grp` whose four cells are the little-endian dword w; an all-air group contributes nothing
__device__ __forceinline__ uint64_t key_map_term(uint32_t grp, uint32_t w) { return w ? key_term(1u, grp, w) : 0ull; }
// the term of inventory entry `item` that holds v; an empty entry contributes nothing
__device__ __forceinline__ uint64_t key_inv_term(uint32_t item, uint32_t v) { return v ? key_term(3u, item, v) : 0ull; }

// XOR over the 16 lanes of a DPP row, left in every lane of it
__device__ __forceinline__ uint32_t key_row_xor(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);   // row_ror:8
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);   // row_ror:4
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);   // row_ror:2
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);   // row_ror:1
    return v;
}

// this lane's share of one row's map and inventory terms (g = lane within the group)
template <int VEC>
__device__ __forceinline__ uint64_t key_row_part(const int8_t* __restrict__ map, const int32_t* __restrict__ inv, int S2, int K, int g, uint32_t fields) {
    typedef uint32_t u32_any __attribute__((aligned(1)));                          // a dword at any byte address
    uint64_t k = 0;
    if (fields & NGW_KEY_MAP) {
        if (VEC == 16) {
            const u32x4* m4 = reinterpret_cast<const u32x4*>(map);
            for (int p = g; p < (S2 >> 4); p += NGW_SNAP_GROUP) {
                const u32x4 v = m4[p];
                const uint32_t g0 = 4u * (uint32_t)p;
                k ^= key_map_term(g0, v.x) ^ key_map_term(g0 + 1u, v.y) ^ key_map_term(g0 + 2u, v.z) ^ key_map_term(g0 + 3u, v.w);
            }
        } else if (VEC == 4) {
            const uint32_t* m1 = reinterpret_cast<const uint32_t*>(map);
            for (int p = g; p < (S2 >> 2); p += NGW_SNAP_GROUP) k ^= key_map_term((uint32_t)p, m1[p]);
        } else {
            const u32_any* m1 = reinterpret_cast<const u32_any*>(map);
            const int nd = S2 >> 2, tail = S2 & 3;
            for (int p = g; p < nd; p += NGW_SNAP_GROUP) k ^= key_map_term((uint32_t)p, m1[p]);
            if (tail && g == (nd & (NGW_SNAP_GROUP - 1))) {                        // the last group's cells, byte by byte; cells past S2 count as 0
                uint32_t w = 0;
                for (int b = 0; b < tail; b++) w |= (uint32_t)(uint8_t)map[4 * nd + b] << (8 * b);
                k ^= key_map_term((uint32_t)nd, w);
            }
        }
    }
    if (fields & NGW_KEY_INV)
        for (int p = g; p < K; p += NGW_SNAP_GROUP) k ^= key_inv_term((uint32_t)p, (uint32_t)inv[p]);
    return k;
}

// VEC = bytes per map piece: 16 / 4 (S2 a multiple of it: every row of every set is that aligned), 1 = odd S2
template <int VEC>
__global__ void __launch_bounds__(NGW_EPB) ngw_keys_kernel(const NgwKeys x) {
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S2 = x.S2, K = x.K;
    const uint32_t fields = x.fields;
    // ---- 1. this lane's row and its scalars
    const bool inside = pair < x.count;
    int si = 0;
    if (inside) si = x.idx ? x.idx[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    const int sic = ok ? si : 0;
    uint64_t key = 0;
    if (fields & NGW_KEY_POSE) {
        const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[sic];
        const int f = x.src.facing[sic];
        key ^= key_term(2u, 0u, (uint32_t)(rc.x | rc.y << 8 | f << 16));
    }
    if (fields & NGW_KEY_SELECTED) key ^= key_term(4u, 0u, (uint32_t)x.src.selected[sic]);
    if (fields & NGW_KEY_STEP_COUNT) key ^= key_term(5u, 0u, (uint32_t)x.src.step_count[sic]);
    if (fields & NGW_KEY_EPISODE) key ^= key_term(6u, 0u, x.src.episode[sic]);
    // ---- 2 / 3. the rows' map and inventory terms, 16 lanes per row
    if (fields & (NGW_KEY_MAP | NGW_KEY_INV)) {
        const int g = (int)(tid % NGW_SNAP_GROUP), q = (int)(tid / NGW_SNAP_GROUP);
#pragma unroll 4
        for (int r = 0; r < NGW_SNAP_GROUP; r++) {
            const int sj = __builtin_amdgcn_ds_bpermute((q * NGW_SNAP_GROUP + r) << 2, sic);
            const uint64_t part = key_row_part<VEC>(x.src.map + (size_t)sj * (size_t)S2, x.src.inv + (size_t)sj * (size_t)K, S2, K, g, fields);
            const uint32_t lo = key_row_xor((uint32_t)part), hi = key_row_xor((uint32_t)(part >> 32));
            if (g == r) key ^= (uint64_t)hi << 32 | lo;
        }
    }
    // ---- 4. lane l holds key l
    if (inside) x.keys[pair] = ok ? key : 0ull;
    if (inside && !ok && si != NGW_IDX_NONE) atomicOr(x.flags, NGW_F_BAD_INDEX);   // (NGW_IDX_NONE: a row that is not there)
}

}  // namespace
