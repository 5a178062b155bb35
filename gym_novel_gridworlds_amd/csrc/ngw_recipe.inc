// ngw_recipe.inc - the recipe heuristic: crafting-cost lower bounds of saved slots and live envs (a unit of its own; host side: ngw_abi_recipe.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// out[j] = the relaxed-plan cost of row idx[j] under the program in the argument block (ngw_device.h NgwRecipe; the contract is include/ngw.h's
// ngw_snapshot_recipe_costs, search.recipe_cost_reference states it in numpy).  What a row contributes is its K inventory words and, for the at
// most four items the program flags, how many cells of its map hold the item.
//
// Shape: the key kernel's (ngw_keys.inc), and no LDS for the maps.  One work-group is one wave: 64 consecutive entries.
//   1. Lane l reads idx[l] (NULL: l), compares it with the row count as an unsigned number and clamps a bad one to row 0 - nothing is ever
//      addressed with the bad index; its cost is 0 and, unless it is NGW_IDX_NONE, NGW_F_BAD_INDEX is raised.
//   2. Only with flagged items (n_map > 0; the Bow program has none and reads no map byte): sixteen rounds of four rows.  NGW_SNAP_GROUP = 16 lanes
//      share one row, consecutive lanes load consecutive 16-byte pieces (S*S a multiple of 16), dwords (a multiple of 4) or - odd S*S - dwords at
//      whatever byte address the row starts and the tail of one to three cells byte by byte.  A row is S*S bytes with no padding behind it: the
//      loops end at S*S, so no byte of the next row is counted.  Each lane counts the bytes of its pieces that equal each flagged item - an integer
//      compare of all four bytes of a dword at once -, two 16-bit counts to a register (a row has at most 4096 cells), and the 16 lanes add them
//      up inside the DPP row with row_ror 8 / 4 / 2 / 1.  Group q = lane / 16 takes row 16 * q + r in round r, its index out of the owner's
//      register with ds_bpermute - -1 for an entry without a row, whose group then loads nothing: the padded tail of a search's child list costs no
//      map read -; lane r of the group keeps the sums: they are where the rules need them.  The branch is around the loads only.
//   3. Lane l runs the rules for row l: the demand per rule lives in LDS, one column per lane ([rule][lane]: a rule number is the same in every
//      lane, so a wave's access is 64 consecutive dwords), the inventory words come from HBM as the rules name them.
// No early exit: every lane is active at every DPP step and every ds_bpermute.

// how many of the four bytes of w equal the byte replicated in c4 (c4 = item * 0x01010101)
__device__ __forceinline__ uint32_t recipe_count4(uint32_t w, uint32_t c4) {
    const uint32_t x = w ^ c4;                                                     // a zero byte where the cell holds the item
    const uint32_t nz = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;      // bit 7 of every byte that is NOT zero
    return 4u - (uint32_t)__popc(nz);
}

// sum over the 16 lanes of a DPP row, left in every lane of it
__device__ __forceinline__ uint32_t recipe_row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);   // row_ror:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);   // row_ror:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);   // row_ror:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);   // row_ror:1
    return v;
}

struct RecipeCounts { uint32_t lo, hi; };   // items 0 | 1 << 16, items 2 | 3 << 16

__device__ __forceinline__ void recipe_count_word(RecipeCounts& c, uint32_t w, const uint32_t (&c4)[4], int n_map) {
    c.lo += recipe_count4(w, c4[0]);
    if (n_map > 1) c.lo += recipe_count4(w, c4[1]) << 16;
    if (n_map > 2) c.hi += recipe_count4(w, c4[2]);
    if (n_map > 3) c.hi += recipe_count4(w, c4[3]) << 16;
}

// this lane's share of one row's counts (g = lane within the group)
template <int VEC>
__device__ __forceinline__ RecipeCounts recipe_row_part(const int8_t* __restrict__ map, int S2, int g, const uint32_t (&c4)[4], int n_map) {
    typedef uint32_t u32_any __attribute__((aligned(1)));                          // a dword at any byte address
    RecipeCounts c = {0u, 0u};
    if (VEC == 16) {
        const u32x4* m4 = reinterpret_cast<const u32x4*>(map);
        for (int p = g; p < (S2 >> 4); p += NGW_SNAP_GROUP) {
            const u32x4 v = m4[p];
            recipe_count_word(c, v.x, c4, n_map); recipe_count_word(c, v.y, c4, n_map);
            recipe_count_word(c, v.z, c4, n_map); recipe_count_word(c, v.w, c4, n_map);
        }
    } else if (VEC == 4) {
        const uint32_t* m1 = reinterpret_cast<const uint32_t*>(map);
        for (int p = g; p < (S2 >> 2); p += NGW_SNAP_GROUP) recipe_count_word(c, m1[p], c4, n_map);
    } else {
        const u32_any* m1 = reinterpret_cast<const u32_any*>(map);
        const int nd = S2 >> 2, tail = S2 & 3;
        for (int p = g; p < nd; p += NGW_SNAP_GROUP) recipe_count_word(c, m1[p], c4, n_map);
        if (tail && g == (nd & (NGW_SNAP_GROUP - 1))) {                            // the last one to three cells, byte by byte: nothing past S2 is read
            for (int b = 0; b < tail; b++) {
                const uint32_t cell = (uint32_t)(uint8_t)map[4 * nd + b];
                c.lo += (uint32_t)(cell == (c4[0] & 255u));
                if (n_map > 1) c.lo += (uint32_t)(cell == (c4[1] & 255u)) << 16;
                if (n_map > 2) c.hi += (uint32_t)(cell == (c4[2] & 255u));
                if (n_map > 3) c.hi += (uint32_t)(cell == (c4[3] & 255u)) << 16;
            }
        }
    }
    return c;
}

// VEC = bytes per map piece: 16 / 4 (S2 a multiple of it: every row of every set is that aligned), 1 = odd S2
template <int VEC>
__global__ void __launch_bounds__(NGW_EPB) ngw_recipe_kernel(const NgwRecipe x) {
    __shared__ int32_t need[NGW_RECIPE_RULES * NGW_EPB];                           // [rule][lane]
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S2 = x.S2, K = x.K;
    const int n_rules = x.prog.n_rules < NGW_RECIPE_RULES ? x.prog.n_rules : NGW_RECIPE_RULES;
    const int n_map = x.prog.n_map < 4 ? x.prog.n_map : 4;
    // ---- 1. this lane's row
    const bool inside = pair < x.count;
    int si = 0;
    if (inside) si = x.idx ? x.idx[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    const int sic = ok ? si : 0;
    // ---- 2. the flagged items on the rows' maps, 16 lanes per row
    RecipeCounts mine = {0u, 0u};
    if (n_map > 0) {
        uint32_t c4[4];
#pragma unroll
        for (int i = 0; i < 4; i++) c4[i] = (uint32_t)x.prog.map_item[i] * 0x01010101u;
        const int g = (int)(tid % NGW_SNAP_GROUP), q = (int)(tid / NGW_SNAP_GROUP);
#pragma unroll 4
        for (int r = 0; r < NGW_SNAP_GROUP; r++) {
            const int sj = __builtin_amdgcn_ds_bpermute((q * NGW_SNAP_GROUP + r) << 2, ok ? si : -1);
            RecipeCounts part = {0u, 0u};                                              // (a row that is not there - a padded list entry - reads no map)
            if (sj >= 0) part = recipe_row_part<VEC>(x.src.map + (size_t)sj * (size_t)S2, S2, g, c4, n_map);
            const uint32_t lo = recipe_row_sum(part.lo), hi = n_map > 2 ? recipe_row_sum(part.hi) : 0u;
            if (g == r) { mine.lo = lo; mine.hi = hi; }
        }
    }
    const int32_t on_map[4] = {(int32_t)(mine.lo & 0xFFFFu), (int32_t)(mine.lo >> 16), (int32_t)(mine.hi & 0xFFFFu), (int32_t)(mine.hi >> 16)};
    // ---- 3. the rules of this lane's row
    const int64_t top = (int64_t)NGW_VALUE_NONE - 1, need_top = 0x7FFFFFFFll;
    for (int r = 0; r < n_rules; r++) need[r * EPB + (int)tid] = r == x.prog.goal_rule ? 1 : 0;
    const int32_t* inv = x.src.inv + (size_t)sic * (size_t)K;
    int64_t h = 0;
    for (int r = 0; r < n_rules; r++) {
        const NgwRecipeRule& u = x.prog.rule[r];
        const int slot = u.map_slot;
        int64_t have = (int64_t)inv[u.out_item < K ? u.out_item : 0];
        if (slot >= 0) have += (int64_t)(slot == 0 ? on_map[0] : (slot == 1 ? on_map[1] : (slot == 2 ? on_map[2] : on_map[3])));
        const int64_t d = (int64_t)need[r * EPB + (int)tid] - have;
        const int64_t qty = u.out_qty ? (int64_t)u.out_qty : 1;
        const int64_t n = d > 0 ? (d + qty - 1) / qty : 0;
        h += n * (int64_t)u.cost;                                                  // (n < 2^31, cost < 2^31, h < 2^31: no wrap)
        h = h > top ? top : h;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int j = u.in_rule[i];
            if (i < (int)u.n_in && j > r && j < n_rules) {                         // (consumers first: an input's rule comes later)
                const int64_t sum = (int64_t)need[j * EPB + (int)tid] + n * (int64_t)u.in_qty[i];
                need[j * EPB + (int)tid] = (int32_t)(sum > need_top ? need_top : sum);
            }
        }
        const int t = u.tool_rule;
        if (t > r && t < n_rules && n > 0 && need[t * EPB + (int)tid] < 1) need[t * EPB + (int)tid] = 1;
    }
    // ---- 4. lane l holds the cost of entry l
    if (inside) x.out[pair] = ok ? (int32_t)h : 0;
    if (inside && !ok && si != NGW_IDX_NONE) atomicOr(x.flags, NGW_F_BAD_INDEX);   // (NGW_IDX_NONE: a row that is not there)
}

}  // namespace
