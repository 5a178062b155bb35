// ngw_sample.inc - the weighted choice among valid actions (the kernel is a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lane_mask, lean_gather_lane, philox_block

namespace {
//
// Two things live here.  The choice itself - sample_choice, rules 3 - 6 of include/ngw.h (ngw_sample_actions), with playout_kth_bit for the
// uniform rule it falls back to - is what ngw_sample_kernel below and ngw_playout_kernel<.., WEIGHTED = true> (ngw_playout.inc) both call:
// there is one statement of the rule on the device.  And ngw_sample_kernel, which applies it once to each of `count` states.
//
// Nothing here restates a game rule: the mask is lane_mask's, the generator is philox_block.

// the id of the (k + 1)-th set bit of m, counted from bit 0 (k < popcount(m)): six halvings, branch-free per lane
__device__ __forceinline__ int playout_kth_bit(uint64_t m, uint32_t k) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const uint32_t below = (uint32_t)__popcll((m >> pos) & ((1ull << width) - 1ull));
        if (k >= below) { pos += width; k -= below; }
    }
    return pos;
}

// Rules 3 - 6: the action for mask word m (never 0: the caller has replaced an empty mask by all A bits) and Philox word w under the weights
// weight_of(a), a < A.  Two walks over the actions with a scalar bound, branch-free per lane: the first sums the cleaned weights (mass), the
// second repeats the sum - the same adds in the same order, so the same c[a] - and keeps the first action whose c[a] exceeds thr = u * mass.
// Every add and multiply is a single rounded binary32 operation (no contraction is possible: no add is fed by a multiply).  A weight that is
// negative, NaN or above 2^64 raises NGW_F_BAD_WEIGHT in `flags`, valid action or not.  mass == 0: the uniform rule on the same w.
template <class WF>
__device__ __forceinline__ int sample_choice(uint64_t m, uint32_t w, int A, const WF& weight_of, float& mass, uint32_t& flags) {
    constexpr float LO = 0x1p-64f, HI = 0x1p64f;
    float c = 0.0f;
    bool bad = false;
    for (int a = 0; a < A; a++) {
        const float x = weight_of(a);
        bad |= !(x >= 0.0f && x <= HI);                                            // (NaN fails both compares; -0.0 passes: it is zero)
        const float v = (((m >> a) & 1ull) && x >= LO && x <= HI) ? x : 0.0f;
        c = __fadd_rn(c, v);
    }
    mass = c;
    if (bad) flags |= NGW_F_BAD_WEIGHT;
    const float u = __fmul_rn((float)(w >> 8), 0x1p-24f);                          // exact: 24 bits
    const float thr = __fmul_rn(u, mass);
    int pick = -1, last = -1;
    c = 0.0f;
    for (int a = 0; a < A; a++) {
        const float x = weight_of(a);
        const float v = (((m >> a) & 1ull) && x >= LO && x <= HI) ? x : 0.0f;
        c = __fadd_rn(c, v);
        const bool pos = v > 0.0f;
        pick = (pos && c > thr && pick < 0) ? a : pick;
        last = pos ? a : last;
    }
    const int weighted = pick < 0 ? last : pick;                                   // (thr < mass always; the fall-back of the contract)
    const int uniform = playout_kth_bit(m, __umulhi(w, (uint32_t)__popcll(m)));
    return mass > 0.0f ? weighted : uniform;
}

// ---------------------------------------------------------------- one weighted choice per state
// ngw_slot_mask_kernel with the choice behind the mask: one lane per pair, 64 pairs per wave.  Lane j reads idx[j] (NULL: j), checks it against
// the row count and CLAMPS a bad one to row 0 - nothing is addressed with the bad one -, gathers the row's pose and inventory
// (lean_gather_lane), reads the map cells the mask needs in place (no LDS staging: every map size), walks lane_mask, then sample_choice over
// its column of the action-major weights: weights[a * stride + j], 256 consecutive bytes per wave and action.  A lane past `count` reads
// column 0 and stores nothing.  A pair whose index was bad stores action -1, mass 0, mask 0 and raises NGW_F_BAD_INDEX.  Nothing but the three
// outputs and the flags word is stored.
template <bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_sample_kernel(const NgwDevSpec* __restrict__ dspec, const NgwSample x, int S, int K) {
    __shared__ int32_t inv_lds[NGW_EPB * (NGW_MAX_ITEMS | 1)];
    const int64_t pair = (int64_t)blockIdx.x * EPB + threadIdx.x;
    const bool inside = pair < (int64_t)x.count;
    int si = 0;
    if (inside) si = x.idx ? x.idx[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    uint32_t flags = (inside && !ok && si != NGW_IDX_NONE) ? NGW_F_BAD_INDEX : 0u;   // (NGW_IDX_NONE: a pair that is not there)
    const LeanLane l = lean_gather_lane(x.src, ok ? si : 0, ok, S, K, inv_lds);
    auto cell_at = [&](int cell) -> int { return (int)ldg<int8_t>(l.bmap, l.mapoff + (uint32_t)cell); };
    const int A = min((int)dspec->u.n_actions, NGW_MAX_ACTIONS);                   // the walks' bound: a scalar
    uint64_t m = lane_mask<EXT>(dspec, S, K, l.r, l.c, l.f, l.sel, l.inv, cell_at);
    if (m == 0) m = (1ull << A) - 1ull;                                            // (A <= 48)
    // the pair's word: key = (lo32(seed), hi32(seed) ^ NGW_SAMPLE_TAG), counter = (t >> 2, 0, lo32(p), hi32(p)) with p = first_pair + j
    const uint64_t p = x.first_pair + (uint64_t)pair;
    uint32_t w0, w1, w2, w3;
    philox_block(x.t >> 2, 0u, (uint32_t)p, (uint32_t)(p >> 32), (uint32_t)x.seed, (uint32_t)(x.seed >> 32) ^ NGW_SAMPLE_TAG, w0, w1, w2, w3);
    const uint32_t qq = x.t & 3u;
    const uint32_t w = qq == 0 ? w0 : (qq == 1 ? w1 : (qq == 2 ? w2 : w3));
    const float* const col = x.weights + (inside ? pair : 0);
    const int64_t stride = x.stride;
    float mass;
    const int action = sample_choice(m, w, A, [&](int a) -> float { return col[(int64_t)a * stride]; }, mass, flags);
    if (inside) {
        x.actions[pair] = ok ? action : -1;
        if (x.mass) x.mass[pair] = ok ? mass : 0.0f;
        if (x.masks) x.masks[pair] = ok ? m : 0ull;
    }
    if (flags) atomicOr(x.flags, flags);
}

}  // namespace
