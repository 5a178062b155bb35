// ngw_path.inc - path keys: the pieces the PATH forms of ngw_slot_rollout_kernel (ngw_slot_rollout.inc) and ngw_playout_kernel
// (ngw_playout.inc) share, and what their launchers check for them (host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lean.inc"            // LeanOut: what a step changed
#include "ngw_keys.inc"            // the terms of a key

namespace {
//
// keys[t * stride + j] = the key ngw_state_keys would return under `fields` for the row pair j is in after it has executed step t (include/ngw.h,
// ngw_snapshot_rollout_path), 0 for a step it did not execute.  A key is an XOR of independent terms, so the T-loop carries it along: the map
// and inventory parts are built once from the lane's staged row and then updated for the dwords a step changed, the scalar terms come from
// registers.  Nothing here restates a hash: the terms are key_term / key_map_term / key_inv_term of ngw_keys.inc.
//   map: lean_body writes the front cell (LeanOut.wcell) and the cells of a pick-up (LeanOut.grab), nothing else.  The dword of the front
//        cell's group is read before the step and - where the step wrote it - after it, and the two terms are swapped.  A pick-up (rare) makes
//        the lanes concerned walk their row again: no second copy of the rows is kept.
//   inventory: Crate, Craft, the slot update and the pick-up write entries LeanOut does not name, so every lane keeps a SHADOW of its K
//        entries (a region of 64 * KP dwords behind the handle's LDS layout), compares the row with it after every step and moves the
//        shadow along - ngw_successors.inc's diff, with "keep" in the place of "undo".

struct PathKeys {
    uint64_t map, inv, episode;                                                    // the running parts; `episode` never changes: the parent's counter
    uint32_t* mrow;                                                                // the lane's map row in LDS, by dwords
    uint32_t* shadow;                                                              // the lane's inventory shadow
    int nd;                                                                        // map groups: (S * S + 3) / 4
    bool k_map, k_inv;
};

// what a lane of a PATH kernel carries through its T-loop; the plain forms carry nothing (their instruction streams are the ones they had)
template <bool PATH>
struct PathLane {};
template <>
struct PathLane<true> {
    PathKeys pk;
    uint64_t* kout;                                                                // this pair's column of x.keys, or nullptr
    int limit;                                                                     // this pair's own bound
    int kdone;                                                                     // the step rows of x.keys written so far
    int grp;                                                                       // the front cell's group of the step under way ...
    uint32_t before;                                                               // ... and its dword before the step
};

__device__ __forceinline__ uint64_t path_map_part(const uint32_t* mrow, int nd) {
    uint64_t k = 0;
    for (int p = 0; p < nd; p++) k ^= key_map_term((uint32_t)p, mrow[p]);
    return k;
}

// after the stage-in's barrier: the cells past S * S of the last group cleared (the contract counts them as 0; the stage-out never reads them),
// the map and inventory parts of the parent's key, the shadow filled
__device__ __forceinline__ PathKeys path_begin(uint32_t* mrow, const int32_t* inv, uint32_t* shadow, int S2, int K, uint32_t fields, uint32_t episode) {
    PathKeys pk;
    pk.mrow = mrow; pk.shadow = shadow; pk.nd = (S2 + 3) >> 2;
    pk.k_map = (fields & NGW_KEY_MAP) != 0; pk.k_inv = (fields & NGW_KEY_INV) != 0;
    pk.map = 0; pk.inv = 0;
    pk.episode = (fields & NGW_KEY_EPISODE) ? key_term(6u, 0u, episode) : 0ull;
    if (pk.k_map) {
        if (S2 & 3) mrow[pk.nd - 1] &= (1u << (8 * (S2 & 3))) - 1u;
        pk.map = path_map_part(mrow, pk.nd);
    }
    if (pk.k_inv)
        for (int p = 0; p < K; p++) {
            const uint32_t v = (uint32_t)inv[p];
            shadow[p] = v;
            pk.inv ^= key_inv_term((uint32_t)p, v);
        }
    return pk;
}

// the group of the cell in front of (r, c, f) - lean_body's fcell - and its dword before the step
__device__ __forceinline__ int path_front_group(const PathKeys& pk, int S, int r, int c, int f, uint32_t& before) {
    const int dr = (f == 0) ? -1 : (f == 1 ? 1 : 0), dc = (f == 2) ? -1 : (f == 3 ? 1 : 0);
    const int grp = min(max(((r + dr) * S + c + dc) >> 2, 0), pk.nd - 1);
    before = pk.k_map ? pk.mrow[grp] : 0u;
    return grp;
}

// the key of the state the running parts and these registers describe: the parts and the scalar terms.  Right behind path_begin, with the
// parent's registers, it is the parent's key - what the GUIDED playout looks up before step 0
__device__ __forceinline__ uint64_t path_key(const PathKeys& pk, uint32_t fields, int r, int c, int f, int sel, int steps) {
    uint64_t key = pk.map ^ pk.inv ^ pk.episode;
    if (fields & NGW_KEY_POSE) key ^= key_term(2u, 0u, (uint32_t)(r | c << 8 | f << 16));
    if (fields & NGW_KEY_SELECTED) key ^= key_term(4u, 0u, (uint32_t)sel);
    if (fields & NGW_KEY_STEP_COUNT) key ^= key_term(5u, 0u, (uint32_t)steps);
    return key;
}

// the step is done: the parts follow the row, and the key of the state it left
__device__ __forceinline__ uint64_t path_after_step(PathKeys& pk, const LeanOut& o, int grp, uint32_t before, const int32_t* inv, int K, uint32_t fields) {
    if (pk.k_map) {
        if (o.wcell) {
            const uint32_t now = pk.mrow[grp];
            if (now != before) pk.map ^= key_map_term((uint32_t)grp, before) ^ key_map_term((uint32_t)grp, now);
        }
        if (__any(o.grab != 0u)) {
            if (o.grab) pk.map = path_map_part(pk.mrow, pk.nd);
        }
    }
    if (pk.k_inv) {
        auto one = [&](int i) {
            const uint32_t wv = (uint32_t)inv[i], sv = pk.shadow[i];
            if (wv != sv) { pk.inv ^= key_inv_term((uint32_t)i, sv) ^ key_inv_term((uint32_t)i, wv); pk.shadow[i] = wv; }
        };
        int i = 0;
        for (; i + 4 <= K; i += 4) {                                               // four entries per test: a step changes a handful of them
            const uint32_t d = ((uint32_t)inv[i] ^ pk.shadow[i]) | ((uint32_t)inv[i + 1] ^ pk.shadow[i + 1]) | ((uint32_t)inv[i + 2] ^ pk.shadow[i + 2]) |
                               ((uint32_t)inv[i + 3] ^ pk.shadow[i + 3]);
            if (d) {
#pragma unroll 1
                for (int j = i; j < i + 4; j++) one(j);
            }
        }
#pragma unroll 1
        for (; i < K; i++) one(i);
    }
    return path_key(pk, fields, o.r, o.c, o.f, o.sel, o.steps);
}

// what the two path launches check beyond the plain ones: a field selection where keys are asked for, a stride that holds the pairs, the shadows inside LDS
inline bool path_args_ok(const NgwLaunch* a, int64_t count, const uint64_t* keys, int64_t keys_stride, uint32_t fields, uint32_t off_shadow, size_t lds_bytes) {
    return (!keys || (fields && !(fields & ~NGW_KEY_ALL) && keys_stride >= count)) && a->KP >= a->K &&
           ((size_t)off_shadow + (size_t)NGW_EPB * (size_t)a->KP) * 4u <= lds_bytes && lds_bytes <= NGW_PATH_LDS_MAX;
}

}  // namespace
