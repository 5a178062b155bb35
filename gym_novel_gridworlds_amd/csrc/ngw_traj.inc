// ngw_traj.inc - trajectories: what the TRAJ forms of ngw_slot_rollout_kernel (ngw_slot_rollout.inc) and ngw_playout_kernel (ngw_playout.inc) add
// to their PATH forms, and what their launchers check for it (host side: ngw_abi_snapshot.cpp).
#pragma once
#include "ngw_common.inc"
#include "ngw_lidar_march.inc"     // lidar_epilogue: the row builder
#include "ngw_path.inc"

namespace {
//
// A learner wants every step of a path, not its sum: the reward of step t, the mask word the choice of step t was made under, and the observation
// before and after it.  The T-loop holds all three - o.reward, m, the state in LDS with the pose in registers -, so the TRAJ forms store them as
// they go: one dword (one qword) per lane and step to [t * stride + pair], 64 lanes on consecutive addresses, and one 64-row LidarInFront tile per
// step, built by lidar_epilogue on the lane's own LDS row and stored to rows (t + 1) * obs_stride + 64 * blockIdx.x .. of x.obs (row block 0: the
// parents).  A step a pair did not execute - its episode is over, its limit is reached, its index was bad - stores 0 and leaves its zeroed tile
// row; the steps behind the wave-uniform early exit are zero-filled as the recorded actions and the keys are.  No row leaves LDS.
//   The launch block of an observing call is the STAND-ALONE lidar launch's layout (ngw_lidar_configure's lidar_proto: item tables | ray table |
// tile | guard | maps | guard | inventory rows), not the rollout layout: lean_body<STAGE = true> and lean_mask_walk take the lane's row pointers
// and never an offset of the block, so they run under either.  The item tables and - where the rays are not world-frame - the 8 KiB per-lane ray
// table are staged ONCE, before the stage-in's barrier (lidar_epilogue on its own would copy the table again at every step).

// what a lane of a TRAJ kernel carries through its T-loop; the other forms carry nothing
template <bool TRAJ>
struct TrajLane {};
template <>
struct TrajLane<true> {
    int32_t* rew;                                                                  // this pair's column of x.rewards, or nullptr
    uint64_t* msk;                                                                 // ... of x.masks (playouts), or nullptr
    int done;                                                                      // the step rows written so far
};

// before the stage-in's barrier: the two item tables and the ray table
__device__ __forceinline__ void traj_obs_begin(const NgwLaunch& a, uint32_t* lds, uint32_t tid) {
    if (tid < LIDAR_ITEM_DW) lds[a.off_litem + tid] = reinterpret_cast<const uint32_t*>(a.lcfg->chan_of_item)[tid];
    if (!a.l_world) lidar_stage_table(a, lds, (int)tid);
}

// this wave's tile of row block `blk` (0: the parents, t + 1: the states step t leaves)
__device__ __forceinline__ char* traj_tile(void* obs, int64_t stride, int blk, int rb) {
    return reinterpret_cast<char*>(obs) + ((uint64_t)blk * (uint64_t)stride + (uint64_t)blockIdx.x * EPB) * (uint64_t)(uint32_t)rb;
}

// one row set: every lane of the wave calls it (barriers inside); `live` = the pair is in the state to observe because it executed the step
__device__ __forceinline__ void traj_obs_rows(const NgwLaunch& a, uint32_t* lds, uint32_t tid, bool live, const int8_t* mp, int S, int r, int c, int f,
                                              const int32_t* inv, void* obs, int64_t stride, int blk) {
    lidar_epilogue(a, lds, (int)tid, live, mp + r * S + c, f, inv, false, true, traj_tile(obs, stride, blk, a.l_rb));
}

// the row blocks of the steps no pair of this wave executed: zeros
__device__ __forceinline__ void traj_zero_tiles(const NgwLaunch& a, uint32_t tid, void* obs, int64_t stride, int from_step, int n_steps) {
    const int npc = 4 * a.l_rb;                                                    // 64 rows = 4 * rb pieces of 16 B
    for (int u = from_step; u < n_steps; u++) {
        GLOBAL_AS u32x4* g4 = (GLOBAL_AS u32x4*)traj_tile(obs, stride, u + 1, a.l_rb);
        for (int p = (int)tid; p < npc; p += EPB) g4[p] = u32x4{0u, 0u, 0u, 0u};
    }
}

// ---------------------------------------------------------------- AgentMap views (x.vw: run-time outputs of the same kernels, no form of their own)
// The observation of ngw_agent_view_kernel for the states of a path: the window of W x W cells around the agent (W = 2 * V + 1, unrotated, 0 outside
// the map), the facing id, the K inventory entries.  The wave's 64 rows of one row block are contiguous in each of the three buffers (the stride is a
// multiple of 64), so a tile is ONE aligned run of 16 * W * W (64, 64 * K) dwords, and lane l stores dword base + l of it: consecutive addresses
// across the wave, whatever W is.  A dword of the window tile lies in at most two rows (W * W >= 9); the lane that builds it fetches those rows'
// agent cells and liveness - packed into one register per lane - with ds_bpermute and reads their map bytes from the wave's maps in LDS (row l at
// l * MS); cells outside the map are masked by bounds on (r, c), never read.  Nothing of this needs LDS of its own: the launch block stays the path
// form's.  Offsets are 64-bit: (T + 1) * stride * W * W exceeds 4 GiB at the large shapes.
__device__ __forceinline__ bool traj_views_on(const NgwTrajViews& v) { return v.view || v.facing || v.inv; }

// the first row of this wave's tile of row block `blk`
__device__ __forceinline__ uint64_t traj_view_row0(const NgwTrajViews& v, int blk) { return (uint64_t)blk * (uint64_t)v.stride + (uint64_t)blockIdx.x * EPB; }

// one row set: every lane of the wave calls it (barriers and ds_bpermute inside); `live` as in traj_obs_rows.  S <= 255 (the maps of a wave fit LDS)
__device__ __forceinline__ void traj_view_rows(const NgwLaunch& a, const NgwTrajViews& v, const uint32_t* lds, uint32_t tid, bool live, int r, int c, int f, int blk) {
    const uint64_t row0 = traj_view_row0(v, blk);
    const int pose = live ? (r | (c << 8) | (1 << 16)) : 0;                        // what the builders of this lane's row need to know of it
    if (v.facing) ((GLOBAL_AS int32_t*)v.facing)[row0 + tid] = live ? f : 0;
    __syncthreads();                                                               // the rows as the other lanes' steps left them
    if (v.view) {
        const int V = v.V, S = a.S, MS = a.MS;
        const uint32_t W = 2u * (uint32_t)V + 1u, WW = W * W, nd = 16u * WW;       // the tile: 64 * W * W bytes
        const int8_t* const maps = reinterpret_cast<const int8_t*>(lds + a.off_map);
        GLOBAL_AS uint32_t* const g = (GLOBAL_AS uint32_t*)(v.view + row0 * (uint64_t)WW);
        for (uint32_t base = 0; base < nd; base += EPB) {                          // (a wave-uniform trip count: ds_bpermute reads every lane)
            const uint32_t p = base + tid;
            const uint32_t idx = min(p, nd - 1u) * 4u;                             // this dword's first byte in the tile
            const uint32_t e = __umulhi(idx, v.magicWW);                           // ... lies in row e of the wave (and its last one in e or e + 1)
            uint32_t rem = idx - e * WW;
            const int p0 = __builtin_amdgcn_ds_bpermute((int)(e << 2), pose);
            const int p1 = __builtin_amdgcn_ds_bpermute((int)(min(e + 1u, (uint32_t)EPB - 1u) << 2), pose);
            int cur = 0;
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t wr = __umulhi(rem, v.magicW), wc = rem - wr * W;
                const int pz = cur ? p1 : p0;
                const int mr = (pz & 255) + (int)wr - V, mc = ((pz >> 8) & 255) + (int)wc - V;
                uint32_t cell = 0;
                if ((pz >> 16) && (unsigned)mr < (unsigned)S && (unsigned)mc < (unsigned)S) cell = (uint8_t)maps[(int)(e + (uint32_t)cur) * MS + mr * S + mc];
                word |= cell << (8 * j);
                if (++rem == WW) { rem = 0; cur = 1; }                             // (the tile's last byte ends row 63: `cur` is not used behind it)
            }
            if (p < nd) g[p] = word;
        }
    }
    if (v.inv) {
        const int K = a.K, KP = a.KP;
        const int32_t* const invs = reinterpret_cast<const int32_t*>(lds + a.off_inv);
        GLOBAL_AS int32_t* const g = (GLOBAL_AS int32_t*)(v.inv + row0 * (uint64_t)(uint32_t)K);
        for (uint32_t i = tid; i < (uint32_t)(EPB * K); i += EPB) {                // (64 * K dwords: every lane runs every round)
            const uint32_t e = __umulhi(i, a.magicK), k = i - e * (uint32_t)K;
            const int pz = __builtin_amdgcn_ds_bpermute((int)(e << 2), pose);
            g[i] = (pz >> 16) ? invs[(int)e * KP + (int)k] : 0;
        }
    }
    __syncthreads();                                                               // (before the next step writes the rows)
}

// the row blocks of the steps no pair of this wave executed: zeros in all three
__device__ __forceinline__ void traj_zero_views(const NgwLaunch& a, const NgwTrajViews& v, uint32_t tid, int from_step, int n_steps) {
    const uint32_t W = 2u * (uint32_t)v.V + 1u, WW = W * W;
    for (int u = from_step; u < n_steps; u++) {
        const uint64_t row0 = traj_view_row0(v, u + 1);
        if (v.view) {
            GLOBAL_AS u32x4* const g4 = (GLOBAL_AS u32x4*)(v.view + row0 * (uint64_t)WW);   // (16-byte aligned: row0 is a multiple of 64)
            for (uint32_t p = tid; p < 4u * WW; p += EPB) g4[p] = u32x4{0u, 0u, 0u, 0u};
        }
        if (v.facing) ((GLOBAL_AS int32_t*)v.facing)[row0 + tid] = 0;
        if (v.inv) {
            GLOBAL_AS int32_t* const g = (GLOBAL_AS int32_t*)(v.inv + row0 * (uint64_t)(uint32_t)a.K);
            for (uint32_t i = tid; i < (uint32_t)(EPB * a.K); i += EPB) g[i] = 0;
        }
    }
}

// the views of one launch as the kernel takes them: the two division magics filled in
inline NgwTrajViews traj_views_ready(NgwTrajViews v) {
    const uint32_t W = 2u * (uint32_t)v.V + 1u;
    v.magicW = (uint32_t)((0x100000000ull + W - 1u) / W);
    v.magicWW = (uint32_t)((0x100000000ull + W * W - 1u) / (W * W));
    return v;
}

// what the two trajectory launches check beyond the plain ones: path_args_ok's list with the shadows only where keys are asked for, strides that
// hold the pairs, and for the observations a whole number of tiles per row block, 16-byte pieces, and the lidar layout inside LDS; for the views
// (never beside the observations) a window size the magics are exact for, whole tiles, 16-byte pieces, and the maps' bytes within a pose's 8 bits
inline bool traj_args_ok(const NgwLaunch* a, int64_t count, const uint64_t* keys, int64_t keys_stride, uint32_t fields, uint32_t off_shadow, size_t lds_bytes,
                         const void* rewards, int64_t rewards_stride, const void* masks, int64_t masks_stride, const void* obs, int64_t obs_stride,
                         const NgwTrajViews& vw) {
    if (a->KP < a->K || lds_bytes > NGW_PATH_LDS_MAX) return false;
    if (keys && !(fields && !(fields & ~NGW_KEY_ALL) && keys_stride >= count && ((size_t)off_shadow + (size_t)NGW_EPB * (size_t)a->KP) * 4u <= lds_bytes)) return false;
    if ((rewards && rewards_stride < count) || (masks && masks_stride < count)) return false;
    if (vw.view || vw.facing || vw.inv) {
        const size_t rows_end = ((size_t)a->off_inv + (size_t)NGW_EPB * (size_t)a->KP) * 4u;
        if (obs || vw.V < 1 || vw.V > NGW_TRAJ_VIEW_MAX || vw.stride % NGW_EPB || vw.stride < blocks_for(count) * NGW_EPB ||
            (reinterpret_cast<uintptr_t>(vw.view) & 15u) || ((reinterpret_cast<uintptr_t>(vw.facing) | reinterpret_cast<uintptr_t>(vw.inv)) & 3u) || a->S > 255 ||
            (size_t)a->off_map * 4u + (size_t)NGW_EPB * (size_t)a->MS > lds_bytes || rows_end > lds_bytes || (keys && rows_end > (size_t)off_shadow * 4u))
            return false;
    }
    if (!obs) return true;
    const size_t tile_end = (size_t)a->off_ltile * 4u + (size_t)NGW_EPB * (size_t)a->l_rb + NGW_EPB;               // (+ one dump byte per lane)
    const size_t rows_end = ((size_t)a->off_inv + (size_t)NGW_EPB * (size_t)a->KP) * 4u;
    return a->lcfg && a->l_rb > 0 && obs_stride % NGW_EPB == 0 && obs_stride >= blocks_for(count) * NGW_EPB && (reinterpret_cast<uintptr_t>(obs) & 15u) == 0 &&
           tile_end <= (size_t)a->off_map * 4u && (size_t)a->off_map * 4u + (size_t)NGW_EPB * (size_t)a->MS <= (size_t)a->off_inv * 4u && rows_end <= lds_bytes &&
           (!keys || rows_end <= (size_t)off_shadow * 4u);
}

}  // namespace
