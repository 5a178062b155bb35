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

// what the two trajectory launches check beyond the plain ones: path_args_ok's list with the shadows only where keys are asked for, strides that
// hold the pairs, and for the observations a whole number of tiles per row block, 16-byte pieces, and the lidar layout inside LDS
inline bool traj_args_ok(const NgwLaunch* a, int64_t count, const uint64_t* keys, int64_t keys_stride, uint32_t fields, uint32_t off_shadow, size_t lds_bytes,
                         const void* rewards, int64_t rewards_stride, const void* masks, int64_t masks_stride, const void* obs, int64_t obs_stride) {
    if (a->KP < a->K || lds_bytes > NGW_PATH_LDS_MAX) return false;
    if (keys && !(fields && !(fields & ~NGW_KEY_ALL) && keys_stride >= count && ((size_t)off_shadow + (size_t)NGW_EPB * (size_t)a->KP) * 4u <= lds_bytes)) return false;
    if ((rewards && rewards_stride < count) || (masks && masks_stride < count)) return false;
    if (!obs) return true;
    const size_t tile_end = (size_t)a->off_ltile * 4u + (size_t)NGW_EPB * (size_t)a->l_rb + NGW_EPB;               // (+ one dump byte per lane)
    const size_t rows_end = ((size_t)a->off_inv + (size_t)NGW_EPB * (size_t)a->KP) * 4u;
    return a->lcfg && a->l_rb > 0 && obs_stride % NGW_EPB == 0 && obs_stride >= blocks_for(count) * NGW_EPB && (reinterpret_cast<uintptr_t>(obs) & 15u) == 0 &&
           tile_end <= (size_t)a->off_map * 4u && (size_t)a->off_map * 4u + (size_t)NGW_EPB * (size_t)a->MS <= (size_t)a->off_inv * 4u && rows_end <= lds_bytes &&
           (!keys || rows_end <= (size_t)off_shadow * 4u);
}

}  // namespace
