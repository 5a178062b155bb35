// ngw_successors.inc - successor keys (a unit of its own; host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // lean_body and its table fetches
#include "ngw_expand.inc"          // expand_rows_in: the gathered stage-in
#include "ngw_keys.inc"            // the terms of a key

namespace {
//
// keys[j * A + a] = the key ngw_state_keys would return under `fields` for the child that ngw_snapshot_expand would write for parent idx[j] and
// action a, for every a in 0 .. A-1 (A = n_actions), and reward / done / info [j * A + a] what that expand would report.  No child is written:
// nothing but the four output arrays and the sticky error flags is stored.  Nothing here restates a game rule or a hash: the step is lean_body,
// the terms are key_term / key_map_term / key_inv_term of ngw_keys.inc, the stage-in is ngw_expand.inc's row mover.
//
// Shape: ngw_expand_kernel's with the stage-out replaced by a loop over the actions.  One work-group is one wave: 64 consecutive parents.
//   1. Lane l reads idx[l] (NULL: l), compares it with the row count as an unsigned number and clamps a bad one to row 0 - nothing is ever
//      addressed with the bad index -, and gathers its parent's pose, selected item, step count and episode counter into registers.  A bad
//      parent (and a lane past `count`) still walks every step below on the row it staged, and stores nothing.
//   2. The wave brings the 64 parent rows into the PRISTINE region of LDS (expand_move_row, 16 lanes per row, one HBM read per row).  The
//      kernel carves its own LDS: two regions of [64 maps, MS bytes apart][64 inventory rows, KP dwords apart] - the handle's row layout, odd
//      dword strides, so 64 lanes that each walk their own row hit distinct banks.
//   3. Barrier; each lane walks its pristine row once: it clears the cells past S*S of the last map group (the contract counts them as 0), copies
//      every dword to the WORK region and XORs the parent's map and inventory terms into `base`.
//   4. For a = 0 .. A-1 (lane l holds entry l of the micro-op table, the loop reads entry a out of lane a with v_readlane: the entry is scalar):
//      lean_body<STAGE = true, WT = false, EXT> on the work row from the parent's scalars; then one pass compares work with pristine dword by
//      dword - over the map groups and the inventory entries -, XORs term(old) out of and term(new) into a copy of `base` where they differ, and
//      writes the pristine dword back.  The pass is the diff and the undo at once and knows nothing of which cells a step may touch.  The
//      scalar terms come from lean_body's outputs (the episode counter is the parent's).  The lane stores key and reports of (l, a).
//   5. One atomicOr raises the flags.
// No early exit: every lane runs every lean_body (it votes with __any) and every readlane.  A lane that is not `ok` runs with live = valid =
// false: the step then picks nothing up and burns nothing, so whatever it writes stays inside its own row.

// One range of a lane's row: for every dword where work differs from pristine, term(i, old) out and term(i, new) in (when `hashed`), and the
// pristine dword back.  Four dwords per test: a step changes a handful of them, so almost every test fails and skips the group.
template <class TERM>
__device__ __forceinline__ uint64_t succ_diff_undo(uint32_t* w, const uint32_t* p, int n, bool hashed, TERM term) {
    uint64_t k = 0;
    auto one = [&](int i) {
        const uint32_t wv = w[i], pv = p[i];
        if (wv != pv) {
            if (hashed) k ^= term((uint32_t)i, pv) ^ term((uint32_t)i, wv);
            w[i] = pv;
        }
    };
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const uint32_t d = (w[i] ^ p[i]) | (w[i + 1] ^ p[i + 1]) | (w[i + 2] ^ p[i + 2]) | (w[i + 3] ^ p[i + 3]);
        if (d) {
#pragma unroll 1
            for (int j = i; j < i + 4; j++) one(j);
        }
    }
#pragma unroll 1
    for (; i < n; i++) one(i);
    return k;
}

// VEC = bytes per map piece in global memory: 16 / 4 (S2 a multiple of it), 1 = odd S2
template <int VEC, bool EXT>
__global__ void __launch_bounds__(NGW_EPB) ngw_successors_kernel(const NgwDevSpec* __restrict__ dspec, const NgwLaunch a, const NgwSuccessors x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const int64_t pair = (int64_t)blockIdx.x * EPB + tid;
    const int S = a.S, K = a.K, S2 = a.S2;
    const uint32_t fields = x.fields;
    // ---- 1. this lane's parent
    const bool inside = pair < x.count;
    int si = 0;
    if (inside) si = x.idx ? x.idx[pair] : (int)pair;
    const bool ok = inside && (uint32_t)si < (uint32_t)x.rows;
    uint32_t flags = (inside && !ok && si != NGW_IDX_NONE) ? NGW_F_BAD_INDEX : 0u;   // (NGW_IDX_NONE: a parent that is not there)
    const int sic = ok ? si : 0;
    const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[sic];
    const int r = rc.x, c = rc.y;
    const int f = x.src.facing[sic];
    const int sel = x.src.selected[sic];
    const int steps = x.src.step_count[sic];
    const uint32_t episode = x.src.episode[sic];
    const LeanTable t = lean_fetch_table(dspec);
    NgwStepU U;
    NgwExtU X;
    lean_fetch_uniforms<EXT>(dspec, U, X);
    if (__ballot(ok) == 0) {                                                       // no live parent in this wave - a frontier's padding: rows of zeros, nothing to stage
        const int A0 = min(U.n_actions, NGW_MAX_ACTIONS);
        if (inside)
            for (int act = 0; act < A0; act++) {
                x.keys[pair * (int64_t)A0 + act] = 0ull;
                if (x.reward) x.reward[pair * (int64_t)A0 + act] = 0;
                if (x.done) x.done[pair * (int64_t)A0 + act] = (uint8_t)0;
                if (x.info) x.info[pair * (int64_t)A0 + act] = 0u;
            }
        if (flags) atomicOr(a.b.flags, flags);
        return;
    }
    // ---- 2. the 64 parent rows into the pristine region
    const int MSdw = a.MS >> 2, KP = a.KP;
    const int region = EPB * (MSdw + KP);                                          // dwords
    uint32_t* const work_map = lds;
    uint32_t* const work_inv = lds + EPB * MSdw;
    uint32_t* const pris_map = lds + region;
    uint32_t* const pris_inv = pris_map + EPB * MSdw;
    expand_rows_in<VEC>(x.src, sic, pris_map, reinterpret_cast<int32_t*>(pris_inv), MSdw, KP, S2, K, tid);
    __syncthreads();
    // ---- 3. this lane's row: pristine -> work, the parent's map and inventory terms
    uint32_t* const wm = work_map + tid * MSdw;
    uint32_t* const wi = work_inv + tid * KP;
    uint32_t* const pm = pris_map + tid * MSdw;
    uint32_t* const pi = pris_inv + tid * KP;
    const int nd = (S2 + 3) >> 2;
    if (S2 & 3) pm[nd - 1] &= (1u << (8 * (S2 & 3))) - 1u;                         // cells past S*S count as 0
    const bool k_map = (fields & NGW_KEY_MAP) != 0, k_inv = (fields & NGW_KEY_INV) != 0;
    uint64_t base = 0;
    for (int p = 0; p < nd; p++) {
        const uint32_t w = pm[p];
        wm[p] = w;
        if (k_map) base ^= key_map_term((uint32_t)p, w);
    }
    for (int p = 0; p < K; p++) {
        const uint32_t v = pi[p];
        wi[p] = v;
        if (k_inv) base ^= key_inv_term((uint32_t)p, v);
    }
    if (fields & NGW_KEY_EPISODE) base ^= key_term(6u, 0u, episode);               // (the child's episode counter is the parent's)
    // ---- 4. every action on the work row, the diff against the pristine row, the undo
    const int A = min(U.n_actions, NGW_MAX_ACTIONS);
    const int64_t out = pair * (int64_t)A;
    for (int act = 0; act < A; act++) {
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)t.t0, act), e1 = (uint32_t)__builtin_amdgcn_readlane((int)t.t1, act);
        const uint32_t e2 = (uint32_t)__builtin_amdgcn_readlane((int)t.t2, act), e3 = (uint32_t)__builtin_amdgcn_readlane((int)t.t3, act);
        const uint32_t e4 = (uint32_t)__builtin_amdgcn_readlane((int)t.t4, act), e5 = (uint32_t)__builtin_amdgcn_readlane((int)t.t5, act);
        const LeanOut o = lean_body<true, false, EXT>(U, X, e0, e1, e2, e3, e4, e5, ok, ok, S, K, reinterpret_cast<int8_t*>(wm), reinterpret_cast<int32_t*>(wi),
                                                      nullptr, nullptr, 0u, 0u, r, c, f, sel, steps, a.autoreset, a.horizon);
        flags |= o.flags;
        uint64_t key = base;
        key ^= succ_diff_undo(wm, pm, nd, k_map, [](uint32_t i, uint32_t w) { return key_map_term(i, w); });
        key ^= succ_diff_undo(wi, pi, K, k_inv, [](uint32_t i, uint32_t v) { return key_inv_term(i, v); });
        if (fields & NGW_KEY_POSE) key ^= key_term(2u, 0u, (uint32_t)(o.r | o.c << 8 | o.f << 16));
        if (fields & NGW_KEY_SELECTED) key ^= key_term(4u, 0u, (uint32_t)o.sel);
        if (fields & NGW_KEY_STEP_COUNT) key ^= key_term(5u, 0u, (uint32_t)o.steps);
        if (inside) {                                                              // (a bad parent: a row of zeros)
            x.keys[out + act] = ok ? key : 0ull;
            if (x.reward) x.reward[out + act] = ok ? o.reward : 0;
            if (x.done) x.done[out + act] = ok ? (uint8_t)o.ended : (uint8_t)0;
            if (x.info) x.info[out + act] = ok ? o.info : 0u;
        }
    }
    // ---- 5. the flags
    if (flags) atomicOr(a.b.flags, flags);
}

}  // namespace
