// ngw_lean.inc — the per-launch step kernel and the fused rollout of everything but the fused lidar epilogue.
#pragma once
#include "ngw_common.inc"
#include "ngw_newepisode.inc"      // new_episode, the Philox sources, the signals towards the host
#include "ngw_lidar_march.inc"     // lidar_epilogue: the fused observation of the staged kernels
#include "ngw_boards.inc"          // lidar_boards_rows: the fused observation of the in-place kernel

namespace {
//
// One launch = one batched step().  Profiling the general kernel (ngw_kernel<., STEP>) with in-kernel clock stamps
// (tools/stamp_timeline.py) showed a wave spending more cycles on loop-invariant address arithmetic hoisted out of its
// cold reset path, on 40 pinned scalars (half of them spilled to VGPR lanes) and on the copy of the action table into
// LDS than on the step itself.  This kernel is the same step written for ONE step and nothing else:
//   * no loop, no lidar epilogue (that configuration keeps the general kernel); the wrapper predicates (FireWall,
//     FenceRestriction, Crate) are a template flag of the same body, behind wave-uniform skips;
//   * the action descriptors never touch LDS: lane l holds the descriptor of action l and each lane fetches its own
//     with ds_bpermute (6 cross-lane reads, no staging, no barrier dependency);
//   * inventory rows go HBM -> registers -> the lane's private LDS row (dynamic slot reads), no transposition;
//   * no per-kind code: an action's 6-dword micro-op entry names the two conditions that make it fail and what a success
//     does; one branch-free body serves every kind (lean_body);
//   * everything a reset needs (placement loop, prepared-episode copy, chunk store-back) lives in ONE out-of-line
//     function that reads its arguments from the HBM blob, so none of its address arithmetic is hoisted into the hot path.
// Semantics and citations are those of ngw_kernel (pogostick_v1_env.py:230-367 etc.); results are bit-identical.
//
// The pieces (each included here, in this order): ngw_lean_cold.inc (helpers, prepared-episode copies, cold paths), ngw_lean_body.inc (the step), ngw_mask.inc (action masks),
// ngw_lean_step.inc (the per-launch kernel + the host write-through form), ngw_lean_rollout.inc (fused rollouts).

#include "ngw_lean_cold.inc"
#include "ngw_lean_body.inc"
#include "ngw_mask.inc"
#include "ngw_lean_step.inc"
#include "ngw_lean_rollout.inc"

}  // namespace
