// ngw_walk.inc - walk distances and go-to plans: shortest paths over (row, column, facing) found in the kernel (a unit of its own; host side:
// ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"

namespace {
//
// Row j of a call: the saved state idx[j] of a set of state rows (a snapshot, or the state slab).  dist[j][k] = the fewest Forward / Left / Right moves
// after which the agent faces a cell of id k, plans[.][j] = the moves of the shortest walk to items[j], length[j] = their number.  The rule is a
// public contract (include/ngw.h, ngw_snapshot_walk): a breadth-first search over the poses (r, c, f) of the static map.
//
// Shape: ONE WAVE IS ONE ROW, one lane is one map row, so a work-group stages one env's planes and not 64 maps - every map size up to 64 x 64 fits
// the default 64 KiB of LDS (below), and the grid supplies the parallelism: at 10 x 10 a CU holds as many work-groups as it has wave slots.
//   1. Every lane reads the row's index (the same address: one scalar load), checks it as an unsigned number - a bad index, or a bad item, is never
//      used as an address: the row's outputs are -1 and NGW_F_BAD_INDEX is raised - and the wave brings the map's S*S bytes into LDS as dwords at
//      whatever byte address the row starts (global memory takes them) and a byte tail.
//   2. Lane r builds the `air` word of map row r (bit c: cell (r, c) holds id 0), as ngw_boards.inc builds occupancy, and keeps four reach words,
//      one per facing: bit c of R[f] = pose (r, c, f) has been reached.  W is uint32_t up to 32 x 32 and uint64_t above.
//   3. One breadth-first layer is one iteration on registers:
//          N' = N | (the row below's N & air) | W | E        S' = S | (the row above's S & air) | W | E
//          W' = W | (W >> 1 & air) | N | S                   E' = E | (E << 1 & air) | N | S
//      (Forward enters a cell only if it is air; a turn stays in its cell: left = {W, E, S, N}, right = {E, W, N, S} of {N, S, W, E}.)  The neighbour
//      rows' words come with ds_bpermute.  Every pose reached FROM layers < d that is not yet reached is layer d exactly, so no frontier is kept.  The
//      layer number of every new bit goes into the uint16 field D[f][r][c] in LDS, lane r writing row r.  The loop ends when a ballot finds no new bit:
//      no fixed bound, no early exit (a serpentine corridor at 32 x 32 takes nearly five hundred layers; 4 * 62 * 62 poses stay below 65 535).
//   4. Lane r walks the set bits of its own reach words once: the id of the cell in front of pose (r, c, f) comes from the staged map, D from the field
//      row the lane wrote itself, and min(D << 16 | r << 10 | c << 4 | f) per id is the distance AND the contract's goal pose (smallest (D, r, c, f)) at
//      once.  Air is the common case and stays in a register, reduced over the wave at the end; the other ids meet in a ds_min_u32 per pose.
//   5. PLANS: the reach words go to LDS, lane 0 walks back from the goal pose - Forward predecessor first, then the Left, then the Right one, each a
//      reach bit and a field entry - and stores move d - 1 of the path for d = length .. 1 where d - 1 < T; the other lanes fill the rest of the column
//      with -1 (disjoint addresses: no store is ordered against another).  The walk is serial: `length` dependent LDS round trips of one lane.
// LDS: the field 8 * S * SP bytes (SP = the row stride in entries: S rounded up so that SP / 2 is odd - lanes that write column c of their rows hit
// distinct banks), the map S*S bytes, the reach words 1 KiB (2 KiB on 64-bit words), the minima 4 * NGW_MAX_ITEMS: 10 x 10 2.0 KiB, 32 x 32 10.6 KiB,
// 64 x 64 39.1 KiB.  No opt-in is needed.

static_assert(NGW_MAX_MAP_SIZE <= 64 && NGW_EPB == 64, "one lane per map row; a pose packs r and c in 6 bits each");

__device__ __forceinline__ int walk_ctz(uint32_t v) { return __builtin_ctz(v); }
__device__ __forceinline__ int walk_ctz(uint64_t v) { return __builtin_ctzll(v); }
// the word lane `src` holds (every lane active)
__device__ __forceinline__ uint32_t walk_from_lane(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
__device__ __forceinline__ uint64_t walk_from_lane(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}
// the tables of the contract: facing NORTH 0, SOUTH 1, WEST 2, EAST 3
__device__ __forceinline__ int walk_dr(int f) { return f == 0 ? -1 : (f == 1 ? 1 : 0); }
__device__ __forceinline__ int walk_dc(int f) { return f == 2 ? -1 : (f == 3 ? 1 : 0); }
// the facing g with left[g] == f is right[f] = {3, 2, 0, 1}, and the one with right[g] == f is left[f] = {2, 3, 1, 0}: two bits per entry
__device__ __forceinline__ int walk_before_left(int f) { return (0x4B >> (2 * f)) & 3; }
__device__ __forceinline__ int walk_before_right(int f) { return (0x1E >> (2 * f)) & 3; }

constexpr uint32_t WALK_NONE = 0xFFFFFFFFu;

template <class W, bool PLANS>
__global__ void __launch_bounds__(NGW_EPB) ngw_walk_kernel(const NgwWalk x) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    __shared__ uint32_t best[NGW_MAX_ITEMS];
    __shared__ W reach[4][NGW_EPB];
    const int lane = (int)threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x;
    const int S = x.S, K = x.K, S2 = S * S, SP = x.SP, T = x.T;
    uint16_t* const field = reinterpret_cast<uint16_t*>(lds);                      // [4][S][SP]
    uint8_t* const lmap = reinterpret_cast<uint8_t*>(lds + 2 * S * SP);            // [S*S]
    // ---- 1. the row, checked; its map into LDS
    const int si = x.idx ? x.idx[j] : (int)j;
    const int item = PLANS ? x.items[j] : 0;
    const bool ok = (uint32_t)si < (uint32_t)x.rows && (uint32_t)item < (uint32_t)K;
    if (!ok) {                                                                     // (uniform: the whole wave leaves)
        if (x.dist && lane < K) x.dist[j * K + lane] = -1;
        if (PLANS) {
            if (x.plans)
                for (int t = lane; t < T; t += EPB) x.plans[(int64_t)t * x.count + j] = -1;
            if (x.length && lane == 0) x.length[j] = -1;
        }
        if (lane == 0 && si != NGW_IDX_NONE && item != NGW_IDX_NONE) atomicOr(x.flags, NGW_F_BAD_INDEX);   // (NGW_IDX_NONE: a row that is not there)
        return;
    }
    const int2 rc = reinterpret_cast<const int2*>(x.src.loc)[si];
    const int r0 = rc.x, c0 = rc.y, f0 = x.src.facing[si];
    const bool pose_ok = (uint32_t)r0 < (uint32_t)S && (uint32_t)c0 < (uint32_t)S && (uint32_t)f0 < 4u;
    {
        typedef uint32_t u32_any __attribute__((aligned(1)));                      // a dword at any byte address
        const uint8_t* const gm = reinterpret_cast<const uint8_t*>(x.src.map) + (size_t)si * (size_t)S2;
        const u32_any* const g1 = reinterpret_cast<const u32_any*>(gm);
        uint32_t* const lm = reinterpret_cast<uint32_t*>(lmap);
        const int nd = S2 >> 2;
        for (int p = lane; p < nd; p += EPB) lm[p] = g1[p];
        if (lane < (S2 & 3)) lmap[4 * nd + lane] = gm[4 * nd + lane];
    }
    if (lane < NGW_MAX_ITEMS) best[lane] = WALK_NONE;
    __syncthreads();
    // ---- 2. this lane's map row as bits, the start pose
    W air = 0;
    if (lane < S)
        for (int c = 0; c < S; c++) air |= (W)(lmap[lane * S + c] == 0) << c;
    W R0 = 0, R1 = 0, R2 = 0, R3 = 0;
    if (pose_ok && lane == r0) {
        const W b = (W)1 << c0;
        R0 = f0 == 0 ? b : 0; R1 = f0 == 1 ? b : 0; R2 = f0 == 2 ? b : 0; R3 = f0 == 3 ? b : 0;
        field[(f0 * S + r0) * SP + c0] = 0;
    }
    // ---- 3. the layers
    uint16_t* const frow = field + lane * SP;                                      // (+ f * S * SP: this lane's row of plane f)
    const int plane = S * SP;
    for (uint32_t d = 1; d < 0xFFFFu; d++) {
        const W below = walk_from_lane(R0, (lane + 1) & 63), above = walk_from_lane(R1, (lane - 1) & 63);
        const W ns = R0 | R1, we = R2 | R3;
        const W n0 = (((lane < 63 ? below : (W)0) & air) | we) & ~R0;
        const W n1 = (((lane > 0 ? above : (W)0) & air) | we) & ~R1;
        const W n2 = (((R2 >> 1) & air) | ns) & ~R2;
        const W n3 = (((R3 << 1) & air) | ns) & ~R3;
        if (__ballot((n0 | n1 | n2 | n3) != 0) == 0) break;
        for (W b = n0; b; b &= b - 1) frow[walk_ctz(b)] = (uint16_t)d;
        for (W b = n1; b; b &= b - 1) frow[plane + walk_ctz(b)] = (uint16_t)d;
        for (W b = n2; b; b &= b - 1) frow[2 * plane + walk_ctz(b)] = (uint16_t)d;
        for (W b = n3; b; b &= b - 1) frow[3 * plane + walk_ctz(b)] = (uint16_t)d;
        R0 |= n0; R1 |= n1; R2 |= n2; R3 |= n3;
    }
    // ---- 4. the nearest pose that faces each id
    uint32_t air_best = WALK_NONE;
    const W R[4] = {R0, R1, R2, R3};
#pragma unroll
    for (int f = 0; f < 4; f++) {
        const int fr = lane + walk_dr(f), dc = walk_dc(f);
        W bits = (uint32_t)fr < (uint32_t)S ? R[f] : (W)0;                         // (a pose whose front cell lies outside the map faces nothing)
        if (dc < 0) bits &= ~(W)1;
        if (dc > 0) bits &= ~((W)1 << (S - 1));
        for (; bits; bits &= bits - 1) {
            const int c = walk_ctz(bits);
            const int id = (int8_t)lmap[fr * S + c + dc];
            const uint32_t key = (uint32_t)frow[f * plane + c] << 16 | (uint32_t)lane << 10 | (uint32_t)c << 4 | (uint32_t)f;
            if (id == 0) air_best = min(air_best, key);
            else if ((uint32_t)id < (uint32_t)K) atomicMin(&best[id], key);
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) air_best = min(air_best, (uint32_t)__shfl_xor((int)air_best, off));
    if (lane == 0) atomicMin(&best[0], air_best);
    if (PLANS) { reach[0][lane] = R0; reach[1][lane] = R1; reach[2][lane] = R2; reach[3][lane] = R3; }
    __syncthreads();
    if (x.dist && lane < K) {
        const uint32_t b = best[lane];
        x.dist[j * K + lane] = b == WALK_NONE ? -1 : (int32_t)(b >> 16);
    }
    if (!PLANS) return;
    // ---- 5. the walk back from the goal pose
    const uint32_t goal = best[item];
    const int len = goal == WALK_NONE ? -1 : (int)(goal >> 16);
    if (x.length && lane == 0) x.length[j] = len;
    if (!x.plans) return;
    for (int t = max(min(len, T), 0) + lane; t < T; t += EPB) x.plans[(int64_t)t * x.count + j] = -1;
    if (lane == 0 && len > 0) {
        int r = (int)(goal >> 10) & 63, c = (int)(goal >> 4) & 63, f = (int)goal & 3;
        // D of a pose inside the map, -1 where it was not reached
        auto D = [&](int pr, int pc, int pf) { return (reach[pf][pr] >> pc) & 1 ? (int)field[(pf * S + pr) * SP + pc] : -1; };
        for (int d = len; d > 0; d--) {
            const int pr = r - walk_dr(f), pc = c - walk_dc(f);
            int act;
            if ((uint32_t)pr < (uint32_t)S && (uint32_t)pc < (uint32_t)S && lmap[r * S + c] == 0 && D(pr, pc, f) == d - 1) { act = x.act_forward; r = pr; c = pc; }
            else if (D(r, c, walk_before_left(f)) == d - 1) { act = x.act_left; f = walk_before_left(f); }
            else { act = x.act_right; f = walk_before_right(f); }
            if (d - 1 < T) x.plans[(int64_t)(d - 1) * x.count + j] = act;
        }
    }
}

}  // namespace
