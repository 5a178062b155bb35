// ngw_select.inc - priority frontiers: the `keep` best candidates of every group of m int32 values, as index lists in the compaction's form (a unit
// of its own; host side: ngw_abi_frontier.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_frontier.inc"     // frontier_wave_prefix, frontier_block_sum

namespace {
//
// The contract is include/ngw.h's (ngw_frontier_select); frontier.select_reference states it in numpy.  A candidate is a position whose value is not
// NGW_VALUE_NONE and whose flag byte, where there are flags, is not zero.  Everything runs on the KEY of a value: uint32(value) ^ 0x80000000 - the
// bias of ngw_table.inc's value words, under which unsigned order is the values' order - and its complement when `largest` is set, so that both modes
// select the SMALLEST keys, the smaller position first among equal ones.  The selection is a radix select: digit by digit from the top, the digit d
// with (keys under the prefix found so far whose digit is below d) < rank <= (... at most d) extends the prefix, and the rank goes on among the keys
// with that digit.  It ends with the threshold key T = the key of the last chosen candidate and r = how many of the keys equal to T are chosen: the
// chosen are the keys below T and the first r, by position, of the keys equal to it.  The entry of a chosen position is (chosen positions before
// it), which comes from counts alone: no atomic orders the output, and the integer atomics below only add counters, whose sums no order changes.
//
// Wave form, m <= NGW_SELECT_WAVE_MAX = 1024, ONE launch.  One wavefront per group (four groups per work-group, no barrier; a wave takes further
// groups in a grid stride when there are more groups than waves).  Lane l holds the keys of positions l, 64 + l, ... (NJ = 4 or 16 registers:
// coalesced loads), so "positions before" is (set lanes of the registers before) + (set lanes below in this one): a ballot, a popcount and an mbcnt.
// The radix select takes one bit per round: per register one ballot of "still under the prefix and this bit clear".  The wave stores its chosen
// entries, NGW_IDX_NONE in [taken, min(keep, m)) of its span, taken[g] and bound[g].  Every wave then adds (1 << 32 | its candidates) to the ticket
// word of the scratch in one atomic; the wave that reads the last ticket stores count[0 .. 2) and puts the word back to 0.  No wave waits.
//
// Grid form, any m up to 2^24, SIX launches behind one hipMemsetAsync of the scratch, over tiles of NGW_FRONTIER_TILE = 4096 positions of one group
// (one work-group of four waves per tile, lane l of the tile holds positions 16 l .. 16 l + 15, as the compaction does):
//   hist<0> .. hist<3>  the histogram of digit P (8 bits, the top byte first) over the tile's candidates under the prefix, in LDS - a wave whose
//                       active keys all share the digit adds once - and from there into the group's 256 counters.  hist<P>, P > 0, first finds digit
//                       P - 1 from the counters the launch before completed: every work-group scans them itself (256 counters, one per thread), and
//                       the group's first tile stores the new prefix and rank for the next launch.  hist<1> also knows the group's candidates:
//                       taken[g] = min(candidates, keep), and their sum over the groups.
//   count               finds the last digit - T and r -, stores bound[g], and the tile's numbers of keys below T and equal to T.
//   scatter             every work-group sums the tiles before its own in its group (at most 4096 pairs), ranks its chosen positions with the
//                       compaction's wave prefixes and stores them; the group's tiles fill [taken, min(keep, m)) of its span; count[0 .. 2).
// What is NGW_IDX_NONE whatever the values are - the entries from min(keep, m) on in every span, and [groups * keep, capacity) - is filled by all
// threads of the wave kernel / the scatter in a grid stride.  A group without a chosen candidate (no candidates, keep == 0) leaves at once in every
// launch.  No position >= n is turned into an address, no entry >= capacity is stored, map is read at p / div for positions p < n only.

constexpr int SEL_BLOCK = NGW_FRONTIER_BLOCK, SEL_WAVES = FR_WAVES;
constexpr int SEL_STATE = 8;                                                       // words of a group's state (ngw_device.h)

__device__ __forceinline__ uint32_t select_key(int32_t v, uint32_t flip) { return ((uint32_t)v ^ 0x80000000u) ^ flip; }
__device__ __forceinline__ int32_t select_value(uint32_t key, uint32_t flip) { return (int32_t)((key ^ flip) ^ 0x80000000u); }
__device__ __forceinline__ uint32_t select_lanes_below(uint64_t b) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// entry e (< capacity) of the lists = position p (< n)
__device__ __forceinline__ void select_store(const NgwSelect& x, int64_t e, int32_t p) {
    const int32_t q = x.div == 1 ? p : p / x.div;
    x.first[e] = x.map ? x.map[q] : q;
    if (x.second) x.second[e] = p - q * x.div;
}
__device__ __forceinline__ void select_none(const NgwSelect& x, int64_t e) {
    x.first[e] = NGW_IDX_NONE;
    if (x.second) x.second[e] = NGW_IDX_NONE;
}

// the entries that hold NGW_IDX_NONE whatever the values are, by thread `gtid` of `threads`
__device__ __forceinline__ void select_fill_static(const NgwSelect& x, int64_t gtid, int64_t threads) {
    for (int64_t e = (int64_t)x.groups * x.keep + gtid; e < x.capacity; e += threads) select_none(x, e);
    const int64_t km = min(x.keep, x.m), extra = (int64_t)x.keep - km;
    if (extra > 0)
        for (int64_t i = gtid; i < extra * x.groups; i += threads) {               // (extra * groups <= groups * keep <= capacity)
            const int64_t g = i / extra;
            select_none(x, g * x.keep + km + (i - g * extra));
        }
}

// ---------------------------------------------------------------------------------------------------------------- the wave form
// grid: at least `work_blocks` work-groups, whose waves take the groups; those behind them only fill
template <int NJ>
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_select_wave_kernel(const NgwSelect x, const int work_blocks) {
    static_assert(NJ * NGW_EPB <= NGW_SELECT_WAVE_MAX && NJ <= 32, "a bit per register in the lane's masks");
    select_fill_static(x, (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x, (int64_t)gridDim.x * SEL_BLOCK);
    if ((int)blockIdx.x >= work_blocks) return;
    const int lane = (int)threadIdx.x & (EPB - 1), n_waves = work_blocks * SEL_WAVES;
    const uint32_t flip = x.largest ? ~0u : 0u;
    const int m = x.m, km = min(x.keep, m);
    uint32_t seen_candidates = 0;
    for (int g = (int)blockIdx.x * SEL_WAVES + (int)threadIdx.x / EPB; g < x.groups; g += n_waves) {     // (uniform in the wave)
        const int64_t base = (int64_t)g * m;
        uint32_t key[NJ], valid = 0, candidates = 0;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int p = j * EPB + lane;
            bool c = false;
            key[j] = 0;
            if (p < m) {
                const int32_t v = x.values[base + p];
                c = v != NGW_VALUE_NONE && (!x.bytes || x.bytes[base + p]);
                key[j] = select_key(v, flip);
            }
            valid |= (uint32_t)c << j;
            candidates += (uint32_t)__popcll(__ballot(c));
        }
        seen_candidates += candidates;
        const uint32_t k = min(candidates, (uint32_t)x.keep);
        uint32_t chosen = 0, T = 0;
        if (k) {
            uint32_t under = valid, need = k;                                      // under: the lane's keys under the prefix T
            for (int bit = 31; bit >= 0; bit--) {
                uint32_t zeros = 0, ones_mask = 0;
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const uint32_t one = (key[j] >> bit) & 1u;
                    ones_mask |= one << j;
                    zeros += (uint32_t)__popcll(__ballot(((under >> j) & 1u) && !one));
                }
                if (need > zeros) {                                                // (uniform) the rank lies among the keys with this bit set
                    need -= zeros;
                    T |= 1u << bit;
                    under &= ones_mask;
                } else {
                    under &= ~ones_mask;
                }
            }
            uint32_t equal_before = 0;                                             // `need` is r now: the keys equal to T that are chosen
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const bool ok = (valid >> j) & 1u, eq = ok && key[j] == T;
                const uint64_t b = __ballot(eq);
                if ((ok && key[j] < T) || (eq && equal_before + select_lanes_below(b) < need)) chosen |= 1u << j;
                equal_before += (uint32_t)__popcll(b);
            }
        }
        const int64_t span = (int64_t)g * x.keep;
        uint32_t before = 0;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const bool c = (chosen >> j) & 1u;
            const uint64_t b = __ballot(c);
            const uint32_t rank = before + select_lanes_below(b);
            if (c && rank < k) select_store(x, span + rank, (int32_t)(base + j * EPB + lane));
            before += (uint32_t)__popcll(b);
        }
        for (int i = (int)k + lane; i < km; i += EPB) select_none(x, span + i);
        if (lane == 0) {
            x.taken[g] = (int32_t)k;
            x.bound[g] = k ? select_value(T, flip) : NGW_VALUE_NONE;
        }
    }
    if (lane == 0) {
        unsigned long long* const word = reinterpret_cast<unsigned long long*>(x.scratch);
        const unsigned long long old = __hip_atomic_fetch_add(word, (1ull << 32) | seen_candidates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(old >> 32) == (uint32_t)n_waves - 1u) {                     // every wave has added its candidates
            const uint32_t all = (uint32_t)old + seen_candidates;
            x.count[0] = x.groups == 1 ? (int32_t)min(all, (uint32_t)x.keep) : x.groups * x.keep;
            x.count[1] = (int32_t)all;
            __hip_atomic_store(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the grid form
__device__ __forceinline__ uint32_t* select_state(const NgwSelect& x, int g) { return x.scratch + 4 + (int64_t)SEL_STATE * g; }
__device__ __forceinline__ uint32_t* select_counters(const NgwSelect& x, int g) { return x.scratch + 4 + (int64_t)SEL_STATE * x.groups + (int64_t)1024 * g; }
__device__ __forceinline__ uint32_t* select_tiles(const NgwSelect& x, int g) {
    return x.scratch + 4 + (int64_t)(SEL_STATE + 1024) * x.groups + (int64_t)2 * g * x.tiles_per_group;
}

// the keys of positions p0 .. p0 + 15 of the group at `base`, and bit i of `valid`: p0 + i is a candidate (a position at or past m: not one)
__device__ __forceinline__ void select_load16(const NgwSelect& x, int64_t base, int p0, uint32_t flip, uint32_t (&key)[16], uint32_t& valid) {
    int32_t v[16];
    uint32_t f = 0xFFFFu;
    if (p0 + 16 <= x.m) {
        const int32_t* src = x.values + base + p0;
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32x4 w = reinterpret_cast<const u32x4*>(src)[j];
                v[4 * j] = (int32_t)w.x; v[4 * j + 1] = (int32_t)w.y; v[4 * j + 2] = (int32_t)w.z; v[4 * j + 3] = (int32_t)w.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = src[i];
        }
        if (x.bytes) {
            f = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) f |= x.bytes[base + p0 + i] ? 1u << i : 0u;
        }
    } else {
        f = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            v[i] = NGW_VALUE_NONE;
            if (p0 + i < x.m) {
                v[i] = x.values[base + p0 + i];
                if (!x.bytes || x.bytes[base + p0 + i]) f |= 1u << i;
            }
        }
    }
    valid = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        key[i] = select_key(v[i], flip);
        if (v[i] != NGW_VALUE_NONE) valid |= f & (1u << i);
    }
}

// A group's 256 counters, one per thread of the work-group: c = counter threadIdx.x, incl = the sum of the counters up to and including it, total =
// their sum (sc: 8 words of LDS; every thread calls it)
__device__ __forceinline__ void select_scan(const uint32_t* counters, uint32_t& c, uint32_t& incl, uint32_t& total, uint32_t* sc) {
    const int tid = (int)threadIdx.x, lane = tid & (EPB - 1), wave = tid / EPB;
    c = counters[tid];
    incl = c;
#pragma unroll
    for (int off = 1; off < EPB; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == EPB - 1) sc[wave] = incl;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; w++) {
        if (w < wave) incl += sc[w];
        total += sc[w];
    }
}

// The digit that holds rank `need` (1-based, 1 <= need <= total) of the counters scanned above: the d with sum(counters[0 .. d)) < need <=
// sum(counters[0 .. d]); need becomes the rank among the keys with that digit.  Every thread calls it and gets the same answer.
__device__ __forceinline__ uint32_t select_digit(uint32_t c, uint32_t incl, uint32_t& need, uint32_t* sc) {
    if (incl >= need && incl - c < need) {                                         // (exactly one thread)
        sc[4] = threadIdx.x;
        sc[5] = need - (incl - c);
    }
    __syncthreads();
    const uint32_t d = sc[4];
    need = sc[5];
    __syncthreads();                                                               // (before sc is written again)
    return d;
}

// grid: groups * tiles_per_group work-groups
template <int PASS>
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_select_hist_kernel(const NgwSelect x) {
    __shared__ uint32_t h[256];
    __shared__ uint32_t sc[8];
    static_assert(SEL_BLOCK == 256, "a thread per counter");
    const int tid = (int)threadIdx.x, lane = tid & (EPB - 1);
    const int g = (int)blockIdx.x / x.tiles_per_group, t = (int)blockIdx.x % x.tiles_per_group;
    uint32_t* const st = select_state(x, g);
    uint32_t* const counters = select_counters(x, g);
    const uint32_t flip = x.largest ? ~0u : 0u;
    uint32_t prefix = 0;
    if constexpr (PASS > 0) {
        uint32_t need = 0, c, incl, total;
        if (PASS > 1) {
            prefix = st[2 * (PASS - 2)];
            need = st[2 * (PASS - 2) + 1];
            if (!need) return;                                                     // (uniform) nothing is chosen in this group
        }
        select_scan(counters + 256 * (PASS - 1), c, incl, total, sc);
        if (PASS == 1) {                                                           // the top byte's counters hold every candidate of the group
            need = (uint32_t)min((int64_t)total, (int64_t)x.keep);
            if (t == 0 && tid == 0) {
                x.taken[g] = (int32_t)need;
                if (!need) x.bound[g] = NGW_VALUE_NONE;
                if (total) atomicAdd(x.scratch + 2, total);
            }
            if (!need) return;
        }
        prefix |= select_digit(c, incl, need, sc) << (32 - 8 * PASS);
        if (t == 0 && tid == 0) {
            st[2 * (PASS - 1)] = prefix;
            st[2 * (PASS - 1) + 1] = need;
        }
    }
    h[tid] = 0;
    __syncthreads();
    uint32_t key[16], valid;
    select_load16(x, (int64_t)g * x.m, t * NGW_FRONTIER_TILE + tid * 16, flip, key, valid);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        bool on = (valid >> i) & 1u;
        if constexpr (PASS > 0) on = on && (key[i] >> (32 - 8 * PASS)) == (prefix >> (32 - 8 * PASS));
        const uint64_t b = __ballot(on);
        if (!b) continue;                                                          // (uniform)
        const uint32_t d = (key[i] >> (24 - 8 * PASS)) & 255u;
        const int lead = __ffsll((unsigned long long)b) - 1;
        const uint32_t d_lead = (uint32_t)__shfl((int)d, lead);
        if (__ballot(on && d == d_lead) == b) {                                    // one digit in the whole wave: one add
            if (lane == lead) atomicAdd(&h[d_lead], (uint32_t)__popcll(b));
        } else if (on) {
            atomicAdd(&h[d], 1u);
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(counters + 256 * PASS + tid, h[tid]);
}

// the lane's 16-bit masks of the keys below T and equal to T
__device__ __forceinline__ void select_masks(const uint32_t (&key)[16], uint32_t valid, uint32_t T, uint32_t& below, uint32_t& equal) {
    below = equal = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        below |= key[i] < T ? 1u << i : 0u;
        equal |= key[i] == T ? 1u << i : 0u;
    }
    below &= valid;
    equal &= valid;
}

// grid: groups * tiles_per_group work-groups
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_select_count_kernel(const NgwSelect x) {
    __shared__ uint32_t sc[8];
    __shared__ int part[FR_WAVES];
    const int tid = (int)threadIdx.x;
    const int g = (int)blockIdx.x / x.tiles_per_group, t = (int)blockIdx.x % x.tiles_per_group;
    uint32_t* const st = select_state(x, g);
    const uint32_t flip = x.largest ? ~0u : 0u;
    uint32_t need = st[5], c, incl, total;
    if (!need) return;                                                             // (uniform)
    select_scan(select_counters(x, g) + 768, c, incl, total, sc);
    const uint32_t T = st[4] | select_digit(c, incl, need, sc);
    if (t == 0 && tid == 0) {
        st[6] = T;
        st[7] = need;
        x.bound[g] = select_value(T, flip);
    }
    uint32_t key[16], valid, below, equal;
    select_load16(x, (int64_t)g * x.m, t * NGW_FRONTIER_TILE + tid * 16, flip, key, valid);
    select_masks(key, valid, T, below, equal);
    const int nb = frontier_block_sum(__popc(below), part), ne = frontier_block_sum(__popc(equal), part);
    if (tid == 0) {
        select_tiles(x, g)[2 * t] = (uint32_t)nb;
        select_tiles(x, g)[2 * t + 1] = (uint32_t)ne;
    }
}

// grid: at least groups * tiles_per_group work-groups (those behind them only fill), at least one
__global__ void __launch_bounds__(NGW_FRONTIER_BLOCK) ngw_select_scatter_kernel(const NgwSelect x) {
    __shared__ int part[FR_WAVES];
    __shared__ int wave_below[FR_WAVES], wave_equal[FR_WAVES];
    const int tid = (int)threadIdx.x, tpg = x.tiles_per_group;
    select_fill_static(x, (int64_t)blockIdx.x * SEL_BLOCK + tid, (int64_t)gridDim.x * SEL_BLOCK);
    if (blockIdx.x == 0 && tid == 0) {
        const uint32_t all = x.scratch[2];
        x.count[0] = x.groups == 1 ? (int32_t)min(all, (uint32_t)x.keep) : x.groups * x.keep;
        x.count[1] = (int32_t)all;
    }
    if ((int64_t)blockIdx.x >= (int64_t)x.groups * tpg) return;
    const int g = (int)blockIdx.x / tpg, t = (int)blockIdx.x % tpg;
    const uint32_t* const st = select_state(x, g);
    const uint32_t T = st[6], r = st[7], flip = x.largest ? ~0u : 0u;
    const int64_t span = (int64_t)g * x.keep;
    const int km = min(x.keep, x.m);
    int64_t k = 0;
    if (r) {                                                                       // (uniform)
        const uint32_t* const tiles = select_tiles(x, g);
        int below_before = 0, equal_before = 0, below_all = 0;
        for (int i = tid; i < tpg; i += SEL_BLOCK) {
            const int nb = (int)tiles[2 * i], ne = (int)tiles[2 * i + 1];
            below_all += nb;
            if (i < t) below_before += nb, equal_before += ne;
        }
        below_before = frontier_block_sum(below_before, part);
        equal_before = frontier_block_sum(equal_before, part);
        k = (int64_t)frontier_block_sum(below_all, part) + r;
        uint32_t key[16], valid, below, equal, wb, we;
        const int p0 = t * NGW_FRONTIER_TILE + tid * 16;
        const int64_t base = (int64_t)g * x.m;
        select_load16(x, base, p0, flip, key, valid);
        select_masks(key, valid, T, below, equal);
        uint32_t nb = frontier_wave_prefix((uint32_t)__popc(below), wb), ne = frontier_wave_prefix((uint32_t)__popc(equal), we);
        const int wave = tid / EPB;
        if ((tid & (EPB - 1)) == 0) wave_below[wave] = (int)wb, wave_equal[wave] = (int)we;
        __syncthreads();
        nb += (uint32_t)below_before;
        ne += (uint32_t)equal_before;
        for (int w = 0; w < wave; w++) nb += (uint32_t)wave_below[w], ne += (uint32_t)wave_equal[w];
        // nb, ne: the keys below T and equal to T at the group's positions before this lane's; the chosen ones among them: nb + min(ne, r)
        for (uint32_t bits = below | equal; bits; bits &= bits - 1) {
            const int i = __builtin_ctz(bits);
            if ((below >> i) & 1u) {
                const int64_t rank = (int64_t)nb + min(ne, r);
                if (rank < k) select_store(x, span + rank, (int32_t)(base + p0 + i));
                nb++;
            } else {
                if (ne < r) select_store(x, span + nb + ne, (int32_t)(base + p0 + i));
                ne++;
            }
        }
    }
    for (int64_t i = k + (int64_t)t * SEL_BLOCK + tid; i < km; i += (int64_t)tpg * SEL_BLOCK) select_none(x, span + i);
}

}  // namespace
