// ngw_device.h — launch descriptors and launcher declarations shared by the device units (ngw_unit_*.hip) and the C-ABI's host side (ngw_abi_*.cpp).
#ifndef NGW_DEVICE_H
#define NGW_DEVICE_H
#include <stdint.h>

#include "../../include/ngw.h"

#define NGW_EPB 64            /* envs per workgroup = one CDNA wavefront, one lane per env */

enum { NGW_MODE_STEP = 0, NGW_MODE_RESET = 1, NGW_MODE_ROLLOUT = 2,
       NGW_MODE_REFILL = 3 /* prepare next episodes in the shadow buffers: a.b = shadow set, a.actions = the main episode[] */,
       NGW_MODE_ROLLOUT_ACT = 4 /* fused rollout with the caller's actions: step t of env e takes a.actions[t * a.t0 + e] */,
       NGW_MODE_DBG_NOP = 8 /* exit at once: launch floor */, NGW_MODE_DBG_COPY = 9 /* stage in/out, no step logic */,
       /* diagnostics: an EMPTY kernel over the same lanes in workgroups of 256 / 1024 / 128 threads (the last with twice the LDS request) ... */
       NGW_MODE_DBG_WG256 = 10, NGW_MODE_DBG_WG1024 = 11, NGW_MODE_DBG_WG128_LDS2 = 12,
       NGW_MODE_DBG_FLOOR = 13 /* ... and in the step kernel's own launch shape (ngw_debug_launch_floor) */ };
/* how a wave's map chunk is laid out in LDS: same image as HBM / odd-dword-padded rows / byte-granular (odd S) */
enum { NGW_MAP_STRAIGHT = 0, NGW_MAP_DWORD = 1, NGW_MAP_BYTE = 2 };

/* Device buffers of one handle.  map/loc/facing/inv are the batched observation AND the state, updated IN PLACE:
 * a step writes through only the bytes it changes (a map cell, a few inventory slots, the agent pose); a reset
 * rewrites the wave's whole chunk with coalesced stores.  Each env is owned by exactly one lane, so there is no
 * intra-launch hazard; launches are ordered by the stream. */
struct NgwBufs {
    int8_t* map;          /* [n_pad][S*S]  */
    int32_t* loc;         /* [n_pad][2]    */
    int32_t* facing;      /* [n_pad]       */
    int32_t* inv;         /* [n_pad][K]    */
    uint8_t* selected;    /* [n_pad] item id, 0 = ''  */
    int32_t* step_count;  /* [n_pad] */
    uint32_t* episode;    /* [n_pad] reset counter, keys the Philox stream */
    int32_t* reward;      /* [n_pad] */
    uint8_t* done;        /* [n_pad] */
    uint32_t* info;       /* [n_pad] packed, see NGW_INFO_* */
    uint32_t* flags;      /* [1] sticky NGW_F_* */
    uint32_t* flags_host; /* single-wavefront handles (host mirror, NgwMirror): the same word in GPU-addressable host memory, or nullptr */
    uint16_t* perm;       /* [S*S][n_pad] shuffle scratch of the subset reset passes, or nullptr */
    uint32_t* brd;        /* [n_pad][BS] occupancy bit rows of the maps (NGW_BOARD_*), part of the state slab; nullptr for maps beyond 32 x 32 */
};

/* Occupancy bit rows ("boards") of a map: word r of an env = bit c set iff map[r][c] != 0, BS = S rounded up to a multiple of 4 words per
 * env (rows >= S are zero), for maps up to 32 x 32.  Auxiliary state of the O(1) LidarInFront observation (ngw_lean.inc, lidar_boards_rows):
 * the in-place step kernel reads a lane's BS words with its prologue loads, cuts the agent's row, column and two diagonals out of them in
 * registers and finds a ray's first block with one find-first-bit - no map in LDS, no march.  Kept coherent by whoever changes a map while
 * the mode is on (NgwLaunch::l_boards): the step kernel's own cell writes, the prepared-episode copies of its cold path, ngw_boards_kernel
 * after every launch that rewrites maps wholesale (resets, refills, rollouts, ngw_set_state). */
#define NGW_BOARD_MAX_S 32
#define NGW_BOARD_STRIDE(S) (((S) + 3) & ~3)

struct NgwLaunch {
    NgwBufs b;
    int64_t n, n_pad, env_base, t0;
    uint64_t seed, action_seed;
    const int32_t* actions;      /* device, NGW_MODE_STEP */
    const uint8_t* reset_mask;   /* device or nullptr, NGW_MODE_RESET */
    int32_t mode, n_steps, autoreset, horizon;
    int32_t S, S2, MS, K, KP, CW; /* MS = LDS bytes per env map (MS/4 odd), KP = K|1 LDS inventory stride, CW = candidate words */
    uint32_t off_map;            /* LDS dword offset of the maps (0, or a guard when the lidar epilogue is fused) */
    /* fused LidarInFront epilogue (kernel template flag LIDAR) */
    const struct NgwLidarDev* lcfg;
    int32_t* lout;               /* [n_pad][lidar_len] */
    int32_t lidar_len, l_beams, l_range, l_chan, l_inv;
    int32_t l_fmt;               /* row format NGW_LFMT_*: int32 / int16 (values saturate at 32767) / packed (uint8 beam entries + int16 inventory tail) */
    int32_t l_world;             /* 1: the ray table is one world-frame table rotated by the facing (NgwLidarDev::woff): wave-uniform ray offsets;
                                  * 2: and it is the reference's default 8-beam table on a NGW_LIDAR_CONST_S map: compile-time offsets */
    int32_t l_rb, l_invoff;      /* bytes per observation row in this format; byte offset of its inventory tail */
    int32_t l_boards;            /* 1: the observation is built from the occupancy bit rows (NgwBufs::brd) by the in-place step kernel / ngw_lidar_boards_kernel */
    int32_t BS;                  /* words per env in NgwBufs::brd (NGW_BOARD_STRIDE(S)), 0 = no boards for this map size */
    uint32_t off_litem;          /* LDS dword offset of the two item tables (chan_of_item | inv_item: 12 dwords) */
    uint32_t off_ltab, off_ltile; /* ... of the per-lane ray table (8 KiB; only when !l_world) and of the observation tile (64 rows, l_rb bytes each) */
    int32_t perm_lds;            /* AddItem shuffle array: 1 = LDS at off_perm ([S2][32] u16, two half-wave batches), 0 = HBM scratch */
    uint32_t off_perm;
    uint32_t magic;              /* ceil(2^32 / (S2/4)) (or / S2 for odd S): exact division of chunk offsets */
    uint32_t magicK;             /* ceil(2^32 / K): exact division of inventory chunk offsets (< 64*K) */
    uint32_t magicS;             /* ceil(2^32 / S): cell / S */
    uint32_t off_inv, off_cand, off_act;    /* LDS dword offsets */
    uint64_t* stamps;            /* diagnostics builds (-DNGW_STAMPS): [grid][16] in-kernel clock stamps, or nullptr */
    uint32_t seq;                /* single-wavefront handles: the step refreshes the host mirror (NgwMirror) and then writes this number to
                                  * flags_host[NGW_SEQ_WORD] (0 = neither) */
    int32_t action0;             /* one-env handles: the step's action travels in the argument block ... */
    int32_t use_action0;         /* ... when this is 1 (`actions` still points at valid device memory); 2: `actions` holds one BYTE per env (ngw_step_host_packed) */
    /* fused rollouts: per-step output rows and per-env episode accumulators (ngw_rollout_outputs), any of them nullptr */
    int32_t* row_reward;         /* [n_steps][row_stride]: reward of step t of env e at [t * row_stride + e] */
    uint8_t* row_done;           /* [n_steps][row_stride]: 1 where the step ended an episode (done, or the horizon under autoreset) */
    int64_t row_stride;
    int32_t* acc;                /* [4][n_pad]: return / length of the running episode, sum of returns / count of the finished ones */
    uint32_t bid0;               /* a per-launch step over a SLICE of the batch: the slice's first block (first env / 64); b.*, actions and the lidar rows
                                  * point at the slice's first env, n is the slice's env count, the cold path adds bid0 to index the blob's unshifted arrays */
};

/* Uniform step parameters: every lane uses the same value, so the kernel reads them with SCALAR loads straight
 * from the HBM blob (no LDS latency in the step's dependency chain). */
struct NgwStepU {
    uint32_t brk_mask, ent_mask, rew_mask;  /* bit i: item i is breakable / an entity / gives break_reward when broken */
    uint32_t brk2_mask;                     /* bit i: breaking item i without an axe yields 2 (BreakIncrease) */
    int32_t n_actions, reward_step, reward_done, break_reward;
    uint8_t cost_forward, cost_turn, cost_break, cost_place, cost_extract, cost_select, table_item, goal_item;
    uint8_t place_item, place_near, n_entities, ext_src, ext_near, ext_out, ext_qty, ext_consume;
    uint8_t ext_cost_ok, axe_item, axe_cost, axe_qty;
    uint8_t cost_chop, cost_jump;
    int8_t chop_reward;
    uint8_t feat;                           /* NGW_FEAT_*: which optional action kinds the spec has (uniform skip of their reads) */
    int8_t place_reward, ext_reward, axe_reward;
    uint8_t axe_required;                   /* AxetoBreak*: Break fails without the selected axe */
    uint32_t _pad64;                        /* 64 bytes: the kernels fetch the struct as 16 dwords with ONE scalar load */
};

enum { NGW_FEAT_JUMP = 1, NGW_FEAT_CHOP = 2 };

/* Lean step kernel (ngw_lean.inc): per-action micro-op table, NGW_LEAN_DW dwords per action, held one action per lane and
 * fetched with ds_bpermute.  A step evaluates a per-lane vector of condition bits NGW_CB_* once; an action names the two
 * conditions that make it fail (outcome s = 1 if A holds, else 2 if B holds, else 0 = success) and carries, per outcome,
 * the message / message argument / cost code, plus what a success does (move, turn, front-cell write, one inventory slot
 * delta, select, reward).  No per-kind code is left in the kernel.
 *   e0 = kind | n_inputs<<4 | needs_table<<7 | arg<<8 | argconst<<16 | is_break<<24
 *   e1 = recipe input item ids (4 bytes, dict order)         e2 = recipe input quantities (4 bytes, 0 beyond n_inputs)
 *   e3 = const slot | cell value<<8 | (int16) slot delta<<16
 *   e4 = A bit | B bit<<4 | msg[0..2]<<8 (4 bits each) | argsel[0..2]<<20 (2 bits each: 0 none, 1 block in front, 2 argconst,
 *        3 recipe<<8|missing mask) | move<<26 (1 front, 2 two ahead) | turn<<28 (1 left, 2 right) | cell write<<30 | select<<31
 *   e5 = reward const (int8) | reward condition bit<<8 | slot select<<12 (0 none, 1 block in front, 2 const slot) | cost[0..2]<<14 (6 bits each)
 * An all-zero entry is a no-op (what an out-of-range action id fetches). */
#define NGW_LEAN_DW 6
enum { NGW_CB_FALSE = 0, NGW_CB_FRONT_NZ = 1, NGW_CB_JUMP_BLOCKED = 2, NGW_CB_NOT_BRK = 3, NGW_CB_NO_PLACE_ITEM = 4, NGW_CB_NOT_SRC = 5,
       NGW_CB_NOT_NEAR = 6, NGW_CB_MISSING = 7, NGW_CB_NEED_TABLE = 8, NGW_CB_NO_ARG_ITEM = 9, NGW_CB_NEED_AXE = 10,
       NGW_CB_NEAR_PLACE = 11, NGW_CB_BRK_REWARD = 12, NGW_CB_TRUE = 13 };

/* Prepared next episodes (ngw_set_reset_prefetch): shadow buffers holding the first states of the next `depth` episodes of
 * every env (depth = dmask + 1, a power of two).  The row of episode E of env e is row (E & dmask) * stride + e of every
 * array, and it is valid iff episode[row] == E; a reset whose new episode number matches copies it instead of running the
 * placement loop.  All null when the feature is off.  Read only on the cold reset path, with scalar loads from the HBM blob. */
#define NGW_MAX_DEPTH 8          /* prepared episodes per env, at most (ngw_set_reset_prefetch_depth) */
#define NGW_SEQ_WORD 8           /* flags_host[8]: sequence number of the last finished step launch (the host polls it instead of a stream sync) */
struct NgwNx {
    int8_t* map;          /* [depth][n_pad][S*S] */
    int32_t* loc;         /* [depth][n_pad][2]   */
    int32_t* facing;      /* [depth][n_pad]      */
    int32_t* inv;         /* [depth][n_pad][K]   */
    uint32_t* episode;    /* [depth][n_pad] episode the row was prepared for (0 = nothing prepared) */
    uint32_t* brd;        /* [depth][n_pad][BS] occupancy bit rows of the prepared maps (valid while the boards mode is on), or nullptr */
    uint32_t* slow;       /* [0] resets that found their row stale and ran the placement loop inside a step (cumulative); [1] refills run so far */
    uint32_t* slow_host;  /* [2] GPU-addressable host words every refill copies `slow` to: the host adapts depth and cadence */
    int64_t stride;       /* rows per slot = n_pad */
    int32_t dmask;        /* depth - 1 */
    int32_t _pad;
};

/* What the cold reset path needs besides the spec: static per handle, read there with scalar loads from the HBM blob
 * (passing them as arguments of the out-of-line reset would spill the call's argument list to scratch). */
struct NgwResetU {
    uint16_t* perm;       /* = NgwBufs.perm */
    int8_t* map;          /* = NgwBufs.map / .inv of the MAIN buffer set: rows a consumed prepared episode is stored to */
    int32_t* inv;
    int64_t n_pad;
    uint64_t seed;
    int32_t S, S2, K, CW, perm_lds;
    uint32_t magicS;
    uint32_t off_rng;     /* LDS dword offset of the Philox word ring [32][64] of the reset path */
    /* the bytes of ngw_spec the reset reads, packed (8 dwords): fetched together with the rest of this struct, so the
     * reset never waits on one more dependent load of the spec for each optional pass */
    uint8_t wall_item, tap_item, tap_near, n_place;
    uint8_t n_passes, n_inv_start, _pad[2];
    uint8_t inv_start_item[NGW_MAX_INV_START], inv_start_qty[NGW_MAX_INV_START];
    uint32_t pass[NGW_MAX_PASSES];         /* kind | item << 8 | from << 16 | percent span << 24 of each shuffled-subset pass */
};

/* Uniform parameters of the step-time novelty predicates (kernel template flag EXT): FireWall, FenceRestriction, Crate */
struct NgwExtU {
    int32_t fire_item, fire_reward, fence_item, fence_mode, crate_item;
    uint32_t crate_add[3];                  /* 4 bits per item id: how many of it a crate holds */
    uint32_t nest;                          /* ngw_spec.ext_flags | fire_skip_recipe << 8 (wrapper nesting of a stack) */
};

/* Blob kept in HBM (one per handle). */
#define NGW_MAX_PLACE 64            /* items placed by one reset (sum of items_quantity); reference: 6-7 */
/* Host mirror of a single-wavefront handle (the gym.Env adapter: n = 1): the same rows in page-locked host memory the GPU
 * addresses directly.  The state itself lives in HBM like any other handle's; a step (or explicit reset) launched by
 * ngw_step_host / ngw_reset_host copies the wave's rows here before it signals completion, so the host reads its results
 * in place - no copy call, no stream synchronisation - and the kernel never READS across PCIe.  All nullptr: no mirror. */
struct NgwMirror {
    int8_t* map; int32_t* loc; int32_t* facing; int32_t* inv; uint8_t* selected; int32_t* step_count;
    int32_t* reward; uint8_t* done; uint32_t* info;
};

/* Terminal observations under same-step autoreset (ngw_set_terminal_capture): before a resetting env's rows are overwritten by its
 * next episode, the step kernel's cold path copies them here - map row, inventory row, pose of the state the episode ENDED in
 * (reference loops look at that observation: tests/test.py:30-41, enjoy.py:107-116).  Row e is valid for the envs whose `done` the
 * same launch set; all null = off (one scalar load and a uniform branch on the cold path, nothing on the hot path). */
struct NgwTerm {
    int8_t* map;          /* [n_pad][S*S] */
    int32_t* loc;         /* [n_pad][2]   */
    int32_t* facing;      /* [n_pad]      */
    int32_t* inv;         /* [n_pad][K]   */
};

/* Host write-through of the step kernel (ngw_step_host_packed's steady state on the in-place kernel): the caller's page-locked block is a
 * mirror of the state and is mapped into the GPU's address space - the step kernel itself stores what the step changes into it across
 * PCIe (the map cells and inventory slots it writes, whole rows of the envs that start a new episode, pose / reward / done / info of every
 * env), counts its finished blocks and the last one publishes the error flags and the launch's sequence number, which the host polls:
 * one launch per host step, no delta kernel behind it, no stream synchronisation.  All null = off. */
struct NgwWT {
    int8_t* map;          /* [n][S*S]  section 0 of the block (device address of the mapped host memory) */
    int32_t* inv;         /* [n][K]    section 1 */
    uint32_t* pose;       /* [n]       section 2: r | c << 8 | facing << 16 | selected << 24 */
    int32_t* reward;      /* [n]       section 3 */
    uint8_t* done;        /* [n]       section 4 */
    uint32_t* info;       /* [n]       section 5 */
    uint32_t* flags;      /* section 6: [0] error flags, [1] sequence number of the last finished step */
    uint32_t* count;      /* device memory: blocks of the current launch that have finished */
    uint8_t* rows;        /* fused LidarInFront observation: the caller's row buffer ([n_pad] rows, ngw_lidar_host_rows), or null */
};

struct NgwDevSpec {
    NgwStepU u;
    uint8_t place_seq[NGW_MAX_PLACE];   /* item id of the n-th placement of a reset (items_quantity flattened in order): the reset paths copy it to LDS */
    int32_t n_place;
    uint32_t act_lean[NGW_MAX_ACTIONS * NGW_LEAN_DW];   /* lean step kernel: micro-op table, see NGW_LEAN_DW */
    NgwLaunch lp;                /* launch prototype (layout + buffer pointers): the lean kernel's cold reset path reads it from here */
    NgwLaunch lp_ns;             /* the same for the no-stage lean kernel (its own, small LDS layout: inventory rows | candidate masks | placement sequence) */
    ngw_spec sp;                 /* full spec: the (cold) reset path reads it with scalar loads */
    NgwExtU x;
    NgwNx nx;
    NgwResetU ru;
    NgwMirror mir;
    NgwTerm term;
    NgwWT wt;
    double pctq[NGW_MAX_PASSES][64];   /* per reset pass: pct / 100.0 for pct in [pct_lo, pct_hi) as the host's IEEE double */
    uint64_t* amask;             /* [n_pad] action masks (ngw_mask.inc): the fused form of the step kernel stores the post-step masks here; nullptr until allocated */
};

/* ngw_launch's `feat`: which instantiation of the kernel that `mode` names the host dispatch (ngw_launch in ngw_unit_general.hip, ngw_part_step in
 * ngw_unit_step_straight.hip) picks. */
enum { NGW_FEAT_LIDAR = 1,    /* fused LidarInFront epilogue (with NGW_FEAT_NOSTAGE: the one on the occupancy bit rows) */
       NGW_FEAT_EXT = 2,      /* wrapper predicates (FireWall / FenceRestriction / Crate) */
       NGW_FEAT_NOSTAGE = 8,  /* NGW_MODE_STEP: the in-place step kernel (maps read where they lie, no staging through LDS) */
       NGW_FEAT_WIRE = 16,    /* ... its host write-through form (NgwWT) */
       NGW_FEAT_MASK = 32,    /* fused action masks (plain steps only: ngw_step_lean<..., MASK>) */
       NGW_FEAT_PLAIN = 64,   /* ... the in-place kernel's instantiation for the plain spec class (ngw_step_plain_class), int32 action rows only */
       NGW_FEAT_VIEW = 128 }; /* ... its form with the fused AgentMap window (ngw_step_lean<..., VIEW>): `a` points at an NgwLaunchView */

/* The launch block of the in-place step kernel's VIEW form: the step's own block, then what the AgentMap epilogue needs (view_rows, ngw_lean_step.inc).
 * The other forms keep NgwLaunch as their argument type, so their argument blocks - and their code - are what they were. */
#define NGW_VIEW_FUSE_MAX 16     /* largest view_size the VIEW form can build (its divisions are exact up to here, as NgwTrajViews') */
#define NGW_VIEW_FUSE_DEFAULT 2  /* ... and the largest one a handle lets it build: one wave builds its 64 windows serially, ~9 instructions per byte, and from
                                  * view_size 5 on that costs more than the second launch saves; NGW_VIEW_FUSE=<view_size> moves it (A/B) */
struct NgwLaunchView : NgwLaunch {
    uint32_t* view;              /* [n][W][W] int8 as n_dwords dwords, W = 2 * V + 1 (ngw_agent_view's buffer) */
    uint32_t n_dwords;
    int32_t V;
    uint32_t magicW, magicWW;    /* ceil(2^32 / W), ceil(2^32 / (W * W)): exact for the operands below 64 * W * W the epilogue divides (V <= NGW_VIEW_FUSE_MAX, as NgwTrajViews) */
};

/* The plain spec class of the in-place step kernel (ngw_step_lean<..., PLAIN>, ngw_lean_step.inc), decided once per handle: at most 12 items
 * (three 16-byte chunks hold an inventory row), no Jump action, no entities, both "near" rules look for the same item, and every byte the hot
 * path addresses lies within 4 GB of its array's scalar base - slab_span: from the state slab's base to the end of its last array over n_pad
 * rows; out_span: the longest of the reward / done / info arrays (allocations of their own) and of the caller's action row.  What a launch adds
 * to it (in place, no wrapper predicates, nothing fused, no write-through, an int32 action row) is the launcher's to check. */
static inline int ngw_step_plain_class(int K, int feat_u /* NgwStepU::feat */, int n_entities, int ext_near, int place_near, uint64_t slab_span, uint64_t out_span) {
    return K >= 4 && K <= 12 && !(feat_u & NGW_FEAT_JUMP) && n_entities == 0 && ext_near == place_near && slab_span < (1ull << 32) && out_span < (1ull << 32);
}
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_launch(const NgwDevSpec* dspec, const NgwLaunch* a, int map_mode, int feat /* NGW_FEAT_* */, unsigned grid, size_t lds_bytes,
                      hipStream_t stream);
/* Arguments of the dedicated new-episode kernel (ngw_reset.inc: explicit resets and prepared next episodes of the plain
 * configurations and of those with ONE subset pass over the air of the interior (AddItem / Crate) or the wall ring (ReplaceItem /
 * FireWall of the wall item)). */
struct NgwResetFast {            // kernel arguments (by value)
    NgwBufs main;                // the handle's state (episode counters; RESET destination)
    NgwNx nx;                    // shadow rows (REFILL destination)
    const uint8_t* reset_mask;   // RESET: device mask or nullptr (all)
    const double* pctq;          // AddItem: pct / 100.0 table of the host
    int64_t n, env_base;
    uint64_t seed;
    uint32_t* flags;
    int32_t mode;                // NGW_MODE_RESET / NGW_MODE_REFILL
    int32_t S, S2, K, CW, n_place, wall_item;
    int32_t additem_item, additem_span;   // the subset pass: item written, width of its percent range
    uint32_t seq;                // single-wavefront handles: refresh the host mirror, then write this to flags_host[NGW_SEQ_WORD] (0 = neither)
    int32_t pass_wall;           // the subset pass replaces WALL cells (ReplaceItem / FireWall of the ring) instead of filling air cells
    int32_t n_inv_start;
    uint32_t inv_start_items, inv_start_qtys;   // 4 bytes each
    uint32_t magicW;             // ceil(2^32 / (S-4))
    uint32_t magicS;             // ceil(2^32 / S)
    int32_t sub_nb, sub_fields;  // subset pass candidates: bits of a cell index (bit_length(S*S - 1)), fields per 32-bit word
    uint32_t magic_tail;         // ceil(2^32 / store units of the last (short) 128-byte window of a row), 0 if S*S % 128 == 0
    uint32_t magicS2;            // ceil(2^32 / (S*S)): byte offset inside the wave's chunk -> env
    int32_t img;                 // rows up to 512 bytes: the LDS tile is the exact image of the wave's 64 rows, stored as one coalesced run
    uint32_t off_ring, off_masks, off_placed, off_tmpl, off_dom, off_mcol, off_tile;    // LDS dword offsets
    uint32_t off_ctab;           // [64] destination rows of a pass (u32) + [64 * NGW_MAX_DEPTH] stale (env, slot) pairs of a compacting refill (u16)
    int32_t boards, BS;          // boards mode: also write the occupancy bit rows (NgwBufs::brd / NgwNx::brd, BS words per env) of every map made or copied
    uint64_t* stamps;            // diagnostics builds (-DNGW_STAMPS), or nullptr
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_reset_fast_launch(const NgwDevSpec* dspec, const struct NgwResetFast* a, int nw, int subset, unsigned grid, size_t lds_bytes,
                                 hipStream_t stream);

/* Row formats of the LidarInFront observation (ngw_lidar_set_output): what one env's row looks like in the device buffer. */
enum { NGW_LFMT_I32 = 0,      /* int32 [B * NC + NI] */
       NGW_LFMT_I16 = 1,      /* int16 [B * NC + NI], values saturate at 32767 */
       NGW_LFMT_PACKED = 2 }; /* uint8 [B * NC] beam entries (a range is <= 64), padded to an even count, then int16 [NI] inventory (saturating) */

/* The reference's DEFAULT LidarInFront rays - 8 beams (observation_wrappers.py:16), i.e. the four axes and the four diagonals, the
 * diagonals advancing by round(0.71 k) cells (np.round(np.cos(pi / 4), 2) = 0.71, :49-55) - as compile-time constants: world ray w
 * (0 .. 7 = +r, +r+c, +c, -r+c, -r, -r-c, -c, +r-c), range k >= 1.  With the map size a compile-time constant too, every cell
 * offset of the march is an instruction immediate.  ngw_lidar_configure compares this table with the host's entry by entry and only
 * an exact match (NgwLaunch::l_world == 2) selects the kernels' constant-offset march. */
#define NGW_LIDAR_CONST_S 10                 /* the map size the constant march is instantiated for: the reference's default */
static constexpr int ngw_lidar8_diag(int k) { return (71 * k + 50) / 100; }        /* round(0.71 k): no tie for k < 50 */
static constexpr int ngw_lidar8_dr(int w, int k) {
    return w == 0 ? k : (w == 4 ? -k : ((w == 1 || w == 7) ? ngw_lidar8_diag(k) : ((w == 3 || w == 5) ? -ngw_lidar8_diag(k) : 0)));
}
static constexpr int ngw_lidar8_dc(int w, int k) {
    return w == 2 ? k : (w == 6 ? -k : ((w == 1 || w == 3) ? ngw_lidar8_diag(k) : ((w == 5 || w == 7) ? -ngw_lidar8_diag(k) : 0)));
}

/* Device-side lidar tables, built by ngw_lidar_configure from ngw_lidar_cfg: flat cell offsets dr * S + dc. */
struct NgwLidarDev {
    int16_t off[4][NGW_LIDAR_MAX_BEAMS][NGW_LIDAR_MAX_RANGE];   /* [facing][beam][range-1], 8 KiB */
    uint8_t chan_of_item[NGW_MAX_ITEMS];
    uint8_t inv_item[NGW_MAX_ITEMS];
    int32_t num_beams, max_range, n_chan, n_inv;
    /* World-frame form of the same table, valid when `world` is set: with num_beams a multiple of 4 the four facings shoot the
     * SAME num_beams directions, only numbered from a different start (observation_wrappers.py:38-43: the angles are
     * direction_radian[facing] - pi + b * 2 pi / B and the four direction_radian values are multiples of 2 pi / 4), so ray b of
     * facing f is world ray (u_f + b - B / 2) mod B with u_f = B / 2, 0, 3 B / 4, B / 4 for NORTH, SOUTH, WEST, EAST.  ngw_lidar_configure
     * checks that property on the host's table entry by entry; the offsets of a ray are then the same for every lane of a wave
     * (scalar loads, no table in LDS).  Ranges beyond max_range repeat the last in-range cell (rows padded to a multiple of 4). */
    int32_t woff[NGW_LIDAR_MAX_BEAMS][NGW_LIDAR_MAX_RANGE];
    int32_t world;
};

#ifdef __cplusplus
extern "C"
#endif
/* Region copies in ONE launch (the "pack" kernel): region r = nbytes[r] bytes from src[r] to dst[r], coalesced 16-byte pieces
 * when both ends are 16-byte aligned.  Three users: the small-batch host step (device regions -> one page-locked host buffer
 * the GPU addresses directly, replacing seven hipMemcpyAsync calls), ngw_pack_obs (the SoA observation / output arrays ->
 * one contiguous payload for the multi-GPU gather) and ngw_unpack_obs (the gathered payloads -> global arrays on the root). */
#define NGW_PACK_MAX 64
struct NgwPack {
    const uint8_t* src[NGW_PACK_MAX];
    uint8_t* dst[NGW_PACK_MAX];
    uint64_t nbytes[NGW_PACK_MAX];
    int32_t n_regions;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_pack_launch(const struct NgwPack* p, hipStream_t stream);
/* Delta refresh of the host mirrors (ngw_step_host on big batches): per region the live array, the device-side shadow of what
 * the host holds, and the host mirror itself as a mapped pointer; pieces of 16 bytes that differ are written to both. */
#define NGW_DIFF_MAX 4
struct NgwDiff {
    const uint8_t* cur[NGW_DIFF_MAX];
    uint8_t* shadow[NGW_DIFF_MAX];
    uint8_t* host[NGW_DIFF_MAX];
    uint64_t nbytes[NGW_DIFF_MAX];
    int32_t n_regions;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_diff_launch(const struct NgwDiff* p, hipStream_t stream);
/* Narrow wire format of the host step (ngw_step_host_packed): per env the pose as four bytes (r, c, facing, selected), the reward as
 * int16, done as a byte and the packed info word, written as four dense arrays into one staging payload that a single copy brings
 * across PCIe (11 B per env instead of the 26 B of the int32 SoA arrays). */
struct NgwWire {
    const int32_t* loc; const int32_t* facing; const uint8_t* selected; const int32_t* reward; const uint8_t* done; const uint32_t* info;
    const uint32_t* flags;
    uint32_t* pose; int32_t* reward32; uint8_t* done8; uint32_t* info32; uint32_t* flags_out;
    int64_t n;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_wire_launch(const struct NgwWire* p, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* delta refresh (NgwDiff) and narrowing (NgwWire) as ONE launch */
hipError_t ngw_diff_wire_launch(const struct NgwDiff* p, const struct NgwWire* w, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* AgentMap window gather: out = [n][2V+1][2V+1] int8 packed as n_dwords dwords */
hipError_t ngw_agent_view_launch(const int8_t* map, const int32_t* loc, uint32_t* out, uint32_t n_dwords, int S, int V,
                                 hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_lidar_launch(const NgwLaunch* a /* with the stand-alone launch's own LDS offsets */, int map_mode, unsigned grid, size_t lds_bytes,
                            hipStream_t stream);
/* Occupancy bit rows (NGW_BOARD_*): rebuild them for `rows` maps (ngw_boards_kernel), and the LidarInFront observation built from them as
 * its own launch (ngw_lidar_boards_kernel) */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_boards_launch(const NgwLaunch* a, int map_mode, const int8_t* map, uint32_t* brd, int64_t rows, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_lidar_boards_launch(const NgwLaunch* a, unsigned grid, size_t lds_bytes, hipStream_t stream);

/* The one-env handle's resident step loop (ngw_solo.inc): kernel arguments.  The kernel stays resident between the steps of a Python loop,
 * speculates the outcome of every action from the committed state into host-visible records, and commits the action the host posts. */
struct NgwSolo {
    NgwBufs b;                   // env 0's rows (the handle's ordinary state arrays)
    volatile uint32_t* mbox;     // host -> device, page-locked host memory: [0] command sequence number, [1] action, [2] quit
    uint32_t* out;               // device -> host, page-locked host memory: [0] sequence of the speculated state, [1] exited, [NGW_SOLO_REC0 ..) records
    int32_t S, S2, K, A, MSp;    // MSp = bytes per private map copy (S2 rounded up to 16)
    uint32_t k0;                 // sequence number of the state the launch starts from
    int32_t commit0;             // an action the host posted while the previous launch was exiting: committed first (-1 = none)
    uint32_t timeout_ticks;      // idle time after which the loop ends (100 MHz ticks)
    uint32_t off_map, off_master, off_inv, off_invb;   // LDS dword offsets: private maps [64][MSp] | master map | inventory rows [64][KP] | their backup
    int32_t KP, rec_dw;          // LDS inventory row stride; dwords per record (8 + K, rounded up to 4)
};
#define NGW_SOLO_REC0 16         // records start at this dword of `out`
// record dwords: [0] reward  [1] info  [2] done | r << 8 | c << 16 | f << 24  [3] selected | wcell << 8 | cell value << 16  [4] step_count
//                [5] cell index of the write  [6] 3 x 3 pick-up mask around the new position  [7] -  [8 ..) the inventory row
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_solo_launch(const NgwDevSpec* dspec, const struct NgwSolo* p, int ext, size_t lds_bytes, hipStream_t stream);
/* Action masks of the state in HBM (ngw_mask.inc): out[e] bit a = step(a) from env e's state would report result == True; [n_pad] words,
 * padding rows 0.  ext: the spec has wrapper predicates (NgwExtU). */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_mask_launch(const NgwDevSpec* dspec, const NgwBufs* b, int64_t n, int S, int K, int ext, uint64_t* out, unsigned grid, hipStream_t stream);

/* One-step lookahead table of the state in HBM (ngw_lookahead.inc): entry (e, a) = reward / done / packed info word that a step of env e with
 * action a would report under the spec and the autoreset setting given; nothing but the table is written.  Action-major: element (e, a) of
 * each array at [a * n_pad + e], padding rows 0; grid = n_pad / NGW_EPB.  ext: the spec has wrapper predicates (NgwExtU). */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_lookahead_launch(const NgwDevSpec* dspec, const NgwBufs* b, int64_t n, int64_t n_pad, int S, int K, int ext, int autoreset, int horizon,
                                int32_t* reward, uint8_t* done, uint32_t* info, unsigned grid, hipStream_t stream);

/* Plan evaluation (ngw_plans.inc, ngw_abi_plans.cpp): n_plans candidate action sequences per env, stepped from the state in HBM on a private
 * copy; nothing but the four result arrays is written.  Results are PLAN-MAJOR: element (e, p) of each array at [p * n_pad + e], padding rows 0.
 * The launch block is the handle's rollout layout with actions = the plans (int32, action of env e, plan p, step t at
 * [(t * n_plans + p) * t0 + e]), t0 = their env stride, n_steps, autoreset, horizon. */
struct NgwPlan {
    int32_t* ret;         /* [n_plans][n_pad] sum of the executed steps' rewards */
    int32_t* length;      /* [n_plans][n_pad] steps executed */
    uint8_t* ended;       /* [n_plans][n_pad] 1: the plan stopped at an episode end */
    uint32_t* info;       /* [n_plans][n_pad] packed info word of the last executed step */
    int32_t n_plans;
    int32_t plan_major;   /* block order: 0 = env-block-major (bid = env_block * n_plans + p), 1 = plan-major (bid = p * env_blocks + env_block) */
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_plans_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwPlan* pa, int map_mode, int ext, size_t lds_bytes, hipStream_t stream);

/* Device-side snapshots (ngw_snapshot.inc, ngw_abi_snapshot.cpp): the seven state arrays of `rows` envs, laid out like the state slab
 * itself (one array per field, row i of every array = one env).  The state slab is the set {map, loc, facing, inv, selected, step_count,
 * episode} of NgwBufs, a snapshot is a second such set of `capacity` rows. */
struct NgwSnapRows {
    int8_t* map;          /* [rows][S*S] */
    int32_t* loc;         /* [rows][2]   */
    int32_t* facing;      /* [rows]      */
    int32_t* inv;         /* [rows][K]   */
    uint8_t* selected;    /* [rows]      */
    int32_t* step_count;  /* [rows]      */
    uint32_t* episode;    /* [rows]      */
};
/* One launch moves `count` rows: dst row di[j] := src row si[j] (a NULL list = j itself).  A row index outside its set makes that one copy
 * a no-op and raises NGW_F_BAD_INDEX in *flags.  keep_episode: dst.episode is left as it is. */
struct NgwSnap {
    NgwSnapRows src, dst;
    const int32_t* si;
    const int32_t* di;
    uint32_t* flags;
    int32_t count, src_rows, dst_rows;
    int32_t S2, K, keep_episode;
};
#define NGW_SNAP_GROUP 16        /* lanes that share one row */
#define NGW_SNAP_BLOCK 256       /* threads per workgroup: 16 rows */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_snapshot_launch(const struct NgwSnap* p, hipStream_t stream);

/* Snapshot expand (ngw_expand.inc, ngw_abi_snapshot.cpp): pair j = row si[j] of `src` (the state slab or a snapshot) stepped once with actions[j],
 * the stepped row - before any reset - stored to row di[j] of `dst` (a snapshot), the step's reward / done / info to element j of the three
 * report arrays (any may be nullptr).  A NULL index list = j itself; an index outside its set skips the pair and raises NGW_F_BAD_INDEX.  src
 * and dst may be the same rows.  The launch block is the handle's rollout layout (LDS carve-up, autoreset, horizon, the flags word). */
struct NgwExpand {
    NgwSnapRows src, dst;
    const int32_t* si;
    const int32_t* di;
    const int32_t* actions;
    int32_t* reward;
    uint8_t* done;
    uint32_t* info;
    int32_t count, src_rows, dst_rows;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_expand_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwExpand* x, int ext, size_t lds_bytes, hipStream_t stream);

/* Snapshot rollout (ngw_slot_rollout.inc, ngw_abi_snapshot.cpp): pair j = row si[j] of `src` (the state slab or a snapshot) stepped up to n_steps
 * times on a private copy with the actions at actions[t * stride + j] (stride >= count), by the rules of the plan kernel: it stops at the first
 * step that ends the episode, that step counts, no reset runs.  ret / length / ended / info (any may be nullptr) take element j as NgwPlan
 * defines them.  keep != 0: the row as the last executed step leaves it goes to row di[j] of `dst` (a snapshot); keep == 0: dst and di are not
 * read and nothing but the reports is stored.  A NULL index list = j itself; an index outside its set skips the pair and raises
 * NGW_F_BAD_INDEX.  src and dst may be the same rows.  The launch block is the handle's rollout layout (LDS carve-up, autoreset, horizon, the
 * flags word). */
/* The AgentMap outputs of a trajectory call (ngw_traj.inc; include/ngw.h ngw_traj_views): any pointer may be nullptr, all three nullptr = no views.
 * view: int8 [n_steps + 1][stride][W * W], W = 2 * V + 1; facing: int32 [n_steps + 1][stride]; inv: int32 [n_steps + 1][stride][K]; row j of block
 * 0 the parent of pair j, of block t + 1 the state step t leaves, zeros for a step the pair did not execute.  stride: rows per block, a multiple of
 * 64 that holds `count` rounded up to 64 - a wave stores its 64 rows of a block as one run of dwords.  magicW / magicWW: ceil(2^32 / W), ceil(2^32 /
 * (W * W)) - exact for the operands below 64 * W * W the kernel divides (V <= NGW_TRAJ_VIEW_MAX); the launchers fill them in. */
struct NgwTrajViews {
    int8_t* view;
    int32_t* facing;
    int32_t* inv;
    int64_t stride;
    int32_t V;
    uint32_t magicW, magicWW;
};

struct NgwSlotRollout {
    NgwSnapRows src, dst;
    const int32_t* si;
    const int32_t* di;
    const int32_t* actions;
    int64_t stride;
    int32_t* ret;
    int32_t* length;
    uint8_t* ended;
    uint32_t* info;
    int32_t count, src_rows, dst_rows;
    int32_t n_steps, keep;
    /* the path form (ngw_path.inc; last: the fields before them keep their offsets).  limits: nullptr, or [count] int32, pair j executes at most
     * min(n_steps, max(limits[j], 0)) steps.  keys: nullptr, or the key under `fields` of the state after step t to keys[t * keys_stride + j]
     * (0 for a step the pair did not execute); off_shadow: the dword offset in LDS of the 64 * KP inventory shadows. */
    const int32_t* limits;
    uint64_t* keys;
    int64_t keys_stride;
    uint32_t fields, off_shadow;
    /* the trajectory form (TRAJ; last again).  rewards: nullptr, or the reward of step t of pair j to rewards[t * rewards_stride + j], 0 for a step the
     * pair did not execute.  obs: nullptr, or the LidarInFront row (the launch block's format, l_rb bytes) of the parent to row j and of the state
     * step t leaves to row (t + 1) * obs_stride + j, all zeros for a step the pair did not execute; obs_stride is a multiple of 64 rows and holds
     * `count` rounded up to 64: a wave stores whole 64-row tiles.  With obs the launch block is the stand-alone lidar launch's layout. */
    int32_t* rewards;
    int64_t rewards_stride;
    void* obs;
    int64_t obs_stride;
    struct NgwTrajViews vw; /* the AgentMap views in the place of obs (last again): the launch block stays the path form's */
};
#define NGW_PATH_LDS_MAX ((size_t)160 * 1024)                                                                   /* what a CU of gfx950 has */
#define NGW_PATH_LDS_BYTES(lds_bytes, KP) ((size_t)(lds_bytes) + (size_t)NGW_EPB * 4u * (size_t)(KP))   /* the handle's layout and the inventory shadows behind it */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_slot_rollout_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* the path form: x->limits / x->keys are read, lds_bytes = NGW_PATH_LDS_BYTES(the handle's, a->KP) with x->off_shadow = the handle's in dwords */
hipError_t ngw_slot_rollout_path_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream);

/* Snapshot playout (ngw_playout.inc, ngw_abi_snapshot.cpp): NgwSlotRollout's pairs, index rules, stop rule and destination, with the actions drawn in
 * the kernel by the choice rule of include/ngw.h (ngw_snapshot_playout): pair j is pair number first_pair + j of the stream of `seed`.  The drawn
 * action of pair j at step t goes to actions[t * stride + j] (nullptr: not recorded; -1 for a step the pair did not execute), the first one to
 * first_action[j].  A skipped pair's reports are stored as 0 and its actions as -1. */
struct NgwPlayout {
    NgwSnapRows src, dst;
    const int32_t* si;
    const int32_t* di;
    int32_t* actions;
    int64_t stride;
    int32_t* ret;
    int32_t* length;
    uint8_t* ended;
    uint32_t* info;
    int32_t* first_action;
    uint64_t seed, first_pair;
    int32_t count, src_rows, dst_rows;
    int32_t n_steps, keep;
    const float* weights; /* nullptr: the uniform rule; else [n_actions] float32, the weighted rule of ngw_sample_actions at every step (last: the fields before it keep their offsets) */
    /* the path form (ngw_path.inc, as in NgwSlotRollout; last: the fields before them keep their offsets).  limits: nullptr, or [count] int32, pair j executes at most
     * min(n_steps, max(limits[j], 0)) steps.  keys: nullptr, or the key under `fields` of the state after step t to keys[t * keys_stride + j]
     * (0 for a step the pair did not execute); off_shadow: the dword offset in LDS of the 64 * KP inventory shadows. */
    const int32_t* limits;
    uint64_t* keys;
    int64_t keys_stride;
    uint32_t fields, off_shadow;
    /* the trajectory form (TRAJ; last again).  rewards: nullptr, or the reward of step t of pair j to rewards[t * rewards_stride + j], 0 for a step the
     * pair did not execute.  obs: nullptr, or the LidarInFront row (the launch block's format, l_rb bytes) of the parent to row j and of the state
     * step t leaves to row (t + 1) * obs_stride + j, all zeros for a step the pair did not execute; obs_stride is a multiple of 64 rows and holds
     * `count` rounded up to 64: a wave stores whole 64-row tiles.  With obs the launch block is the stand-alone lidar launch's layout. */
    int32_t* rewards;
    int64_t rewards_stride;
    uint64_t* masks;      /* nullptr, or the mask word the choice of step t was made under (after the all-actions replacement) to masks[t * masks_stride + j], 0 likewise */
    int64_t masks_stride;
    void* obs;
    int64_t obs_stride;
    struct NgwTrajViews vw; /* the AgentMap views in the place of obs (last again): the launch block stays the path form's */
    /* the guided form (GUIDED; last again; read by ngw_playout_guided_launch alone).  tkey: the key[] array of a key table of tmask + 1 buckets (a power
     * of two), only read.  table_weights: float32 [tmask + 1][tw_stride], row b the weights of the steps taken from the state bucket b holds; a state
     * the table does not hold draws by `weights` (nullptr: the uniform rule) or, with stop != 0, ends the pair there as a limit would.  where: nullptr,
     * or the bucket of the state pair j was in before step t to where[t * where_stride + j], -1 for a miss and for a step the pair did not execute;
     * depth: nullptr, or [count], the leading executed steps with where >= 0.  fields is never 0 and the shadows lie behind the layout whether or not
     * keys is set: the running key is what is looked up. */
    const uint64_t* tkey;
    uint64_t tmask;
    const float* table_weights;
    int32_t* where;
    int64_t where_stride;
    int32_t* depth;
    int32_t tw_stride, stop;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_playout_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* the path form, as ngw_slot_rollout_path_launch */
hipError_t ngw_playout_path_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* the trajectory forms (PATH and TRAJ): x->rewards / x->masks / x->obs are read too.  Without x->obs: the path launch's block and lds_bytes.  With
 * it: a = the stand-alone lidar launch's layout (ngw_lidar_configure) with a->autoreset, a->horizon, x->off_shadow behind it where x->keys is
 * set, lds_bytes = that layout's (+ the shadows).  With x->vw (and no x->obs): the handle's rollout layout, lds_bytes = the handle's (+ the shadows
 * where x->keys is set); vw.magicW / vw.magicWW are the launcher's to fill */
hipError_t ngw_slot_rollout_traj_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwSlotRollout* x, int ext, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_playout_traj_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* the guided form (PATH, TRAJ and GUIDED): ngw_playout_traj_launch's block and lds_bytes with the shadows ALWAYS behind the layout (x->off_shadow), and
 * x->tkey / x->tmask / x->table_weights / x->tw_stride / x->stop read; x->fields is a non-empty selection whether or not x->keys is set */
hipError_t ngw_playout_guided_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwPlayout* x, int ext, size_t lds_bytes, hipStream_t stream);

/* Slot observations (ngw_slot_observe.inc, ngw_abi_snapshot.cpp): observations and action masks of SAVED states, gathered by slot index. Output
 * row j of a call describes row slots[j] of `src` (a snapshot; a NULL list = j itself).  An index outside [0, rows) is never used as an address:
 * its output row is all zeros and NGW_F_BAD_INDEX is raised in *flags.  Nothing but the output rows and the flags word is stored.  The three
 * kernels share the struct; the fields behind `rows` are the agent-view gather's. */
struct NgwSlotObs {
    NgwSnapRows src;
    const int32_t* slots;
    uint32_t* flags;
    int32_t count, rows;
    uint32_t* view;       /* [count][W][W] int8 as n_dwords dwords, or nullptr */
    int32_t* facing;      /* [count], or nullptr */
    int32_t* inv;         /* [count][K], or nullptr */
    uint32_t n_dwords, magicW;
    int32_t S, K, V;
};
#ifdef __cplusplus
extern "C"
#endif
/* a = the stand-alone lidar launch's layout (ngw_lidar_configure) with a.lout = the caller's rows ([count rounded up to 64] rows of the current format) */
hipError_t ngw_slot_lidar_launch(const NgwLaunch* a, const struct NgwSlotObs* x, size_t lds_bytes, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_slot_view_launch(const struct NgwSlotObs* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
/* out[j] = the mask word of slot slots[j] ([count] words; ngw_mask.inc's predicate) */
hipError_t ngw_slot_mask_launch(const NgwDevSpec* dspec, const struct NgwSlotObs* x, int S, int K, int ext, uint64_t* out, hipStream_t stream);

/* The weighted choice (ngw_sample.inc, ngw_abi_snapshot.cpp): for pair j < count, row idx[j] of `src` (a snapshot or the state slab; a NULL list = j
 * itself) gets one action drawn by the rule of include/ngw.h (ngw_sample_actions) from the weights weights[a * stride + j] (stride >= count), as pair
 * number first_pair + j of the stream of `seed` at step number t.  actions[j] int32, mass[j] float32 and masks[j] (mass, masks: may be nullptr).
 * An index outside [0, rows) is never used as an address: its outputs are -1 / 0 / 0 and NGW_F_BAD_INDEX is raised in *flags; a bad weight
 * raises NGW_F_BAD_WEIGHT.  Nothing but the three outputs and the flags word is stored. */
struct NgwSample {
    NgwSnapRows src;
    const int32_t* idx;
    const float* weights;
    int64_t stride;
    uint64_t seed, first_pair;
    uint32_t* flags;
    int32_t* actions;
    float* mass;
    uint64_t* masks;
    int32_t count, rows;
    uint32_t t;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_sample_launch(const NgwDevSpec* dspec, const struct NgwSample* x, int S, int K, int ext, hipStream_t stream);

/* State keys (ngw_keys.inc, ngw_abi_snapshot.cpp): keys[j] = the 64-bit key (include/ngw.h, ngw_state_keys) of row idx[j] of `src` (a snapshot or the
 * state slab; a NULL list = j itself) under the field selection `fields` (NGW_KEY_*).  An index outside [0, rows) is never used as an address: its
 * key is 0 and NGW_F_BAD_INDEX is raised in *flags.  Nothing but keys[0 .. count) and the flags word is stored. */
struct NgwKeys {
    NgwSnapRows src;
    const int32_t* idx;
    uint32_t* flags;
    uint64_t* keys;
    int64_t count;
    int32_t rows, S2, K;
    uint32_t fields;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_keys_launch(const struct NgwKeys* x, hipStream_t stream);

/* Successor keys (ngw_successors.inc, ngw_abi_snapshot.cpp): for parent j = row idx[j] of `src` (a snapshot or the state slab; a NULL list = j itself)
 * and every action a of the spec, keys[j * A + a] = the key under `fields` of the row ngw_expand_kernel would store for (j, a), and reward / done /
 * info [j * A + a] (any may be nullptr) what it would report.  An index outside [0, rows) is never used as an address: its A keys and reports are 0
 * and NGW_F_BAD_INDEX is raised.  Nothing but [0, count * A) of the given arrays and the flags word is stored.  The launch block is the handle's
 * (S, K, MS, KP, autoreset, horizon, the flags word); the kernel keeps two sets of 64 rows in LDS, carved by itself. */
struct NgwSuccessors {
    NgwSnapRows src;
    const int32_t* idx;
    uint64_t* keys;
    int32_t* reward;
    uint8_t* done;
    uint32_t* info;
    int64_t count;
    int32_t rows;
    uint32_t fields;
};
#define NGW_SUCC_LDS_BYTES(MS, KP) ((size_t)2 * NGW_EPB * ((size_t)(MS) + 4u * (size_t)(KP)))   /* a work and a pristine set of 64 rows */
#define NGW_SUCC_LDS_MAX ((size_t)160 * 1024)                                                    /* what a CU of gfx950 has */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_successors_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwSuccessors* x, int ext, hipStream_t stream);

/* Walk distances and go-to plans (ngw_walk.inc, ngw_abi_snapshot.cpp): for row j = row idx[j] of `src` (a snapshot or the state slab; a NULL list = j
 * itself), dist[j * K + k] = the fewest Forward / Left / Right moves until the agent faces a cell of id k (-1: never) under the rule of include/ngw.h
 * (ngw_snapshot_walk); with items != nullptr also length[j] = dist[j][items[j]] and plans[t * count + j] = move t of that walk for t < min(length, T), -1
 * elsewhere (act_forward / act_left / act_right: the ids stored).  dist, and with items plans and length, may be nullptr.  An index outside [0, rows), or
 * an item outside [0, K), is never used as an address: the row's outputs are all -1 and NGW_F_BAD_INDEX is raised in *flags.  Nothing but the three
 * outputs and the flags word is stored.  One work-group - one wave - per row: grid = count. */
struct NgwWalk {
    NgwSnapRows src;
    const int32_t* idx;
    const int32_t* items;   /* [count], or nullptr: distances only (T, plans, length are then not read) */
    uint32_t* flags;
    int32_t* dist;          /* [count][K] */
    int32_t* plans;         /* [T][count] */
    int32_t* length;        /* [count] */
    int64_t count;
    int32_t rows, S, K, T;
    int32_t SP;             /* NGW_WALK_SP(S) */
    int32_t act_forward, act_left, act_right;
};
/* the row stride of the kernel's uint16 distance field: S rounded up to an even number of entries whose half is odd (lanes l and l + 1 then write
 * the same column of their rows to different banks), and the dynamic LDS of a launch: the field [4][S][SP] and the map's S*S bytes as dwords */
#define NGW_WALK_SP(S) (((((S) + 1) >> 1) | 1) << 1)
#define NGW_WALK_LDS_BYTES(S) ((size_t)8 * (size_t)(S) * (size_t)NGW_WALK_SP(S) + (((size_t)(S) * (size_t)(S) + 3u) & ~(size_t)3))
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_walk_launch(const struct NgwWalk* x, hipStream_t stream);

/* Key table (ngw_table.inc, ngw_abi_table.cpp): an open-addressing set of 64-bit keys in device memory.  key[] and stamp[] hold mask + 1 words
 * (a power of two); key 0 marks an empty bucket, a stamp is the smallest base + position that ever offered the bucket's key (all ones: none yet).
 * One insert is two launches: the probe places or finds keys[j], writes its bucket to where[j] (-1: key 0, or no bucket left - NGW_F_TABLE_FULL in
 * *flags) and lowers the bucket's stamp to base + j; the second launch sets fresh[j] = (stamp[where[j]] == base + j).  A lookup probes with plain
 * loads and stores nothing but where[0 .. count).  `fresh` is not read by the probe and may be nullptr for a lookup. */
struct NgwTable {
    uint64_t* key;
    uint64_t* stamp;
    unsigned long long* stored;   /* keys in the table */
    uint32_t* flags;
    const uint64_t* keys;         /* [count] */
    int32_t* where;               /* [count] */
    uint8_t* fresh;               /* [count] */
    uint64_t base, mask;
    int64_t count;
    /* a valued table's insert_min (read by ngw_table_insert_min_launch alone; last, so that the arguments of insert and lookup lie where they lay).
     * best[]: mask + 1 words (uint32(value) ^ 0x80000000) << 32 | low half of the base + j that offered it, all ones = never valued; tag[]: mask + 1
     * int32.  The probe also lowers best[where[j]] to position j's word unless values[j] is NGW_VALUE_NONE; the second launch sets improved[j] =
     * (best[where[j]] == that word) and, where it is set and tags != nullptr, tag[where[j]] = tags[j].  The host keeps the low halves growing:
     * (uint32)base + count <= 2^32 in every launch (ngw_table_renorm_launch before the call that would pass it). */
    uint64_t* best;
    int32_t* tag;
    const int32_t* values;        /* [count] */
    const int32_t* tags;          /* [count], or nullptr */
    uint8_t* improved;            /* [count] */
};
#define NGW_TABLE_BLOCK 256      /* threads per workgroup: four waves, one key per lane */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_insert_launch(const struct NgwTable* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_lookup_launch(const struct NgwTable* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_insert_min_launch(const struct NgwTable* x, hipStream_t stream);
/* every valued word of best[0 .. buckets) keeps its value and gets the low half 0 */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_renorm_launch(uint64_t* best, uint64_t buckets, hipStream_t stream);

/* value[j], tag_out[j] = the value and the tag of bucket where[j] of a valued table; (NGW_VALUE_NONE, NGW_TAG_ROOT) for a bucket outside [0, mask],
 * which also raises NGW_F_BAD_INDEX in *flags unless it is -1 or NGW_IDX_NONE.  One lane per query, one launch. */
struct NgwTableRead {
    const uint64_t* best;
    const int32_t* tag;
    uint32_t* flags;
    const int32_t* where;         /* [count] */
    int32_t* value;               /* [count] */
    int32_t* tag_out;             /* [count] */
    uint64_t mask;
    int64_t count;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_read_launch(const struct NgwTableRead* x, hipStream_t stream);

/* The chain of tags = parent_bucket * A + action from bucket where[j] to a bucket whose tag is NGW_TAG_ROOT, as a plan: plans[t * count + j] = move t
 * for t < length[j], -1 behind it, root[j] = the bucket the chain ends in.  At most T links are followed: a longer chain (a cycle), where[j] of -1 or
 * NGW_IDX_NONE -> length = root = -1 and a column of -1; a bucket outside the table, an empty one or a tag outside [0, (mask + 1) * A) likewise, and
 * NGW_F_BAD_INDEX in *flags.  (mask + 1) * A <= 2^31 - 1.  One lane per query, one launch. */
struct NgwTableTrace {
    const uint64_t* key;
    const int32_t* tag;
    uint32_t* flags;
    const int32_t* where;         /* [count] */
    int32_t* plans;               /* [T][count] */
    int32_t* length;              /* [count] */
    int32_t* root;                /* [count] */
    uint64_t mask;
    int64_t count;
    int32_t T, A;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_table_trace_launch(const struct NgwTableTrace* x, hipStream_t stream);

/* Frontiers (ngw_frontier.inc, ngw_abi_frontier.cpp): flags -> an index list of fixed capacity, and slots for it, without the host knowing how many.
 * Compaction: the positions p with bytes[p] != 0 in ascending order, the k-th of them to first[k] = (map ? map[p / div] : p / div) and second[k] =
 * p % div for k < min(total, capacity), NGW_IDX_NONE behind them up to capacity, count[0] = the entries written, count[1] = total; total > capacity
 * raises NGW_F_FRONTIER_FULL in *flags.  Two launches: the count of every tile of NGW_FRONTIER_TILE bytes to tiles[0 .. n_tiles), then the scatter,
 * in which every work-group sums the tiles before its own (and all of them) itself.  Nothing else is stored. */
struct NgwFrontier {
    const uint8_t* bytes;   /* [n] */
    const int32_t* map;     /* [ceil(n / div)], or nullptr: the identity */
    int32_t* first;         /* [capacity] */
    int32_t* second;        /* [capacity], or nullptr */
    int32_t* count;         /* [2] */
    int32_t* tiles;         /* [n_tiles]: the handle's scratch */
    uint32_t* flags;
    int64_t n, capacity;
    int32_t div, n_tiles;
};
/* Slot allocation: c = *cursor, m = max(min(count[0], limit - c), 0); slots[k] = c + k for k < m and NGW_IDX_NONE for m <= k < capacity; *cursor = c + m,
 * written by the work-group that takes the last ticket - after every work-group has read it -, which also puts *ticket back to 0; m < count[0]
 * raises NGW_F_FRONTIER_FULL. */
struct NgwFrontierAlloc {
    const int32_t* count;
    int32_t* cursor;
    int32_t* slots;         /* [capacity] */
    uint32_t* ticket;       /* one word of the handle's scratch, 0 between the calls */
    uint32_t* flags;
    int64_t capacity;
    int32_t limit;
};
#define NGW_FRONTIER_BLOCK 256                         /* threads per workgroup: four waves, 16 flag bytes per lane */
#define NGW_FRONTIER_TILE (16 * NGW_FRONTIER_BLOCK)    /* flag bytes per workgroup */
#define NGW_FRONTIER_MAX_FLAGS (1ll << 24)             /* the longest flag array of one call: 4096 tiles, whose counts every work-group of the scatter sums */
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_frontier_compact_launch(const struct NgwFrontier* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_frontier_alloc_launch(const struct NgwFrontierAlloc* x, hipStream_t stream);

/* Priority frontiers (ngw_select.inc, ngw_abi_frontier.cpp): the `keep` best candidates of each of `groups` groups of m int32 values, in the list
 * form of the compaction.  The contract is include/ngw.h's (ngw_frontier_select); frontier.select_reference states it in numpy.  A candidate is a
 * position p with values[p] != NGW_VALUE_NONE and (bytes == nullptr or bytes[p] != 0); the selection runs on the key uint32(value) ^ 0x80000000,
 * complemented when `largest` is set, smallest key first and the smaller position first among equal keys.  Two forms, picked by
 * ngw_frontier_select_launch alone: m <= NGW_SELECT_WAVE_MAX one wavefront per group and ONE launch; above it the grid form of SIX launches over
 * tiles of NGW_FRONTIER_TILE positions (four digit histograms, the tiles' counts, the scatter), behind one hipMemsetAsync of the scratch.
 * scratch (uint32 words, NGW_SELECT_SCRATCH_WORDS(groups, tiles_per_group) of them for the grid form, 2 for the wave form; 8-byte aligned):
 *   [0 .. 2)  the wave form's ticket word (64 bits: waves arrived << 32 | candidates so far), 0 between the calls - the last wave puts it back
 *   [2]       the grid form's candidates over all groups             [3] unused
 *   [4 + 8 g .. )                       group g: (key prefix, rank still looked for under it) after the first, second and third digit, then (T, r):
 *                                       the threshold key and how many of the keys equal to it are chosen; r == 0: nothing is chosen in the group
 *   [4 + 8 groups + 1024 g + 256 d ..)  group g, digit d (0 = the top byte): 256 counters
 *   [4 + 1032 groups + 2 (g tpg + t) ..)  tile t of group g: the keys below the threshold, the keys equal to it */
struct NgwSelect {
    const int32_t* values;  /* [groups * m] */
    const uint8_t* bytes;   /* [groups * m], or nullptr: every position */
    const int32_t* map;     /* [ceil(groups * m / div)], or nullptr: the identity */
    int32_t* first;         /* [capacity] */
    int32_t* second;        /* [capacity], or nullptr */
    int32_t* taken;         /* [groups] */
    int32_t* bound;         /* [groups] */
    int32_t* count;         /* [2] */
    uint32_t* scratch;      /* the handle's */
    int64_t capacity;       /* >= groups * keep */
    int32_t groups, m, div, keep, largest;
    int32_t tiles_per_group;    /* ceil(m / NGW_FRONTIER_TILE) */
};
#define NGW_SELECT_WAVE_MAX 1024                       /* the largest group one wavefront selects from: 16 values per lane */
#define NGW_SELECT_MAX_VALUES (1ll << 24)              /* the most values (and the most groups) of one call */
#define NGW_SELECT_SCRATCH_WORDS(groups, tpg) (4ll + 1032ll * (groups) + 2ll * (groups) * (tpg))
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_frontier_select_launch(const struct NgwSelect* x, hipStream_t stream);

/* Search runs (ngw_search.inc, ngw_abi_search.cpp): the glue of one best-first iteration between the five existing stages, as three kernels of one
 * thread per position.  The contract is include/ngw.h's (ngw_search_run); search.relax_reference states the three in numpy.  n = capacity * A
 * positions, position q = j * A + a: parent entry j, action a.
 *   offer   values[q] = g[parents[j]] + cost, tags[q] = bucket[parents[j]] * A + a.  cost = lut[a] (by_action) or lut[NGW_INFO_COST(info[q])].  No
 *           offer - values[q] = NGW_VALUE_NONE, tags[q] = NGW_TAG_ROOT - for a parent that is NGW_IDX_NONE or outside [0, pool), a g of
 *           NGW_VALUE_NONE, and a sum outside [INT32_MIN, NGW_VALUE_NONE): the last is counted in row[NGW_SEARCH_OVERFLOW] and *overflowed.
 *   judge   row[NGW_SEARCH_IMPROVED] += the positions with best[q] != 0; such a position whose info word has NGW_INFO_DONE and a message code other
 *           than 14 lowers *goal to (uint32(values[q]) ^ 0x80000000) << 32 | uint32(where[q]) - the minimum taken inside the wave, one atomic per
 *           wave that has one.  stop: best[q] = 0 wherever NGW_INFO_DONE(info[q]) is set.
 *   settle  entry k < capacity of the chosen (first[k] = j, second[k] = a) and slots[k] = c: plist[k] = parents[j] (NGW_IDX_NONE for a padded
 *           entry); where the entry and its slot are live, g[c] = values[j * A + a], bucket[c] = where[j * A + a] and next[k] = c, else next[k] =
 *           NGW_IDX_NONE.  row[NGW_SEARCH_EXPANDED] += the live ones; thread 0 zero-fills next_row, the stats row of the following iteration.
 * No index is used as an address unchecked: j against capacity, parents[j] and c against pool. */
struct NgwSearch {
    const int32_t* parents;     /* [capacity] */
    int32_t* next;              /* [capacity]: the other parent list */
    int32_t* g;                 /* [pool] */
    int32_t* bucket;            /* [pool] */
    const uint32_t* info;       /* [n] */
    const int32_t* lut;         /* [64] */
    int32_t* values;            /* [n] */
    int32_t* tags;              /* [n] */
    const int32_t* where;       /* [n] */
    uint8_t* best;              /* [n] */
    const int32_t* first;       /* [capacity] */
    const int32_t* second;      /* [capacity] */
    const int32_t* slots;       /* [capacity] */
    int32_t* plist;             /* [capacity] */
    unsigned long long* goal;   /* one word, all ones: no goal yet */
    unsigned long long* overflowed;
    uint32_t* row;              /* [4]: this iteration's stats */
    uint32_t* next_row;         /* [4]: the next one's */
    int64_t capacity, pool;
    int32_t A, by_action, stop;
    /* an open-list search (below); all NULL / 0 in a closed one, whose kernels read none of them */
    int32_t* f;                 /* [pool]: the priority of every open slot, NGW_VALUE_NONE elsewhere */
    int32_t* h;                 /* [pool]: the heuristic of the state in every slot */
    int32_t* slot_of_bucket;    /* [buckets]: the slot that holds the cheapest copy of the bucket's state, -1: none */
    const int32_t* dist;        /* [capacity][K]: ngw_snapshot_walk of the child list; NULL: no heuristic */
    const int32_t* weights;     /* [K] */
    const int32_t* sel_count;   /* ngw_frontier_select's count words of this iteration's choice */
    uint32_t* orow;             /* [8]: this iteration's row of the open-list stats */
    uint32_t* next_orow;        /* [8]: the next one's */
    int64_t buckets;
    int32_t K, mode, prune;
    const int32_t* recipe;      /* [capacity]: the recipe term of every entry of the child list (ngw_recipe_launch); NULL: none, h is the walk term alone */
};
#define NGW_SEARCH_BLOCK 256     /* threads per workgroup: four waves, one position per lane */
#define NGW_SEARCH_OFFERED 0     /* the columns of a stats row */
#define NGW_SEARCH_IMPROVED 1
#define NGW_SEARCH_EXPANDED 2
#define NGW_SEARCH_OVERFLOW 3
/* Open-list searches (ngw_search_create_open; the contract is include/ngw.h's "an open-list iteration"; search.take_reference, .open_reference and
 * .best_first_reference state the kernels in numpy).  Two kernels more, and the settle and roots kernels instantiated with the open-list work:
 *   take    entry k < capacity of the chosen list P = parents (ngw_frontier_select's `first` over f): a slot in [0, pool) is CLOSED - f[slot] =
 *           NGW_VALUE_NONE -; with prune, an old f >= the goal word's value makes P[k] = NGW_IDX_NONE.  orow: CHOSEN += the slots, PRUNED += the pruned
 *           ones, FMIN / FBOUND = the smallest / largest old f (signed; one atomicMin / atomicMax per wave that has a slot); thread 0 stores
 *           orow[OPEN] = sel_count[1].
 *   settle  as above, and for a live child c with bucket b = where[q] in [0, buckets): an earlier slot named by slot_of_bucket[b] gets f =
 *           NGW_VALUE_NONE and is counted in orow[SUPERSEDED]; slot_of_bucket[b] = c.  Thread 0 resets next_orow as well.
 *   open    entry k < capacity of the child list `next`: a slot c in [0, pool) gets h[c] = the walk heuristic of dist[k][0 .. K) (0 without one)
 *           and f[c] = min(int64(g[c]) + h[c], NGW_VALUE_NONE - 1).
 *   roots   as below with parents[j] = NGW_IDX_NONE for every j; a root taken (best[j] set) gets slot_of_bucket[where[j]] = r, h[r] from dist[j]
 *           and f[r] as in open.
 * The walk heuristic of K distances d under K weights w >= 0: min (mode NGW_SEARCH_H_MIN) or max (NGW_SEARCH_H_MAX) of int64(w[k]) * d[k] over the k
 * with w[k] > 0 and d[k] >= 0, clamped to NGW_VALUE_NONE - 1; 0 where there is no such k. */
#define NGW_SEARCH_CHOSEN 0      /* the columns of an open-list stats row (8 words) */
#define NGW_SEARCH_PRUNED 1
#define NGW_SEARCH_SUPERSEDED 2
#define NGW_SEARCH_OPEN 3
#define NGW_SEARCH_FMIN 4        /* int32; NGW_VALUE_NONE until a slot is chosen */
#define NGW_SEARCH_FBOUND 5      /* int32; INT32_MIN until a slot is chosen */
#define NGW_SEARCH_OPEN_COLS 8
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_take_launch(const struct NgwSearch* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_open_launch(const struct NgwSearch* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_offer_launch(const struct NgwSearch* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_judge_launch(const struct NgwSearch* x, hipStream_t stream);
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_settle_launch(const struct NgwSearch* x, hipStream_t stream);
/* the roots of a search (ngw_search_start): for j < count, a root slot r = roots[j] in [0, pool) with where[j] >= 0 gets g[r] = value[j] and bucket[r] =
 * where[j]; parents[j] = r where best[j] != 0, NGW_IDX_NONE otherwise and for count <= j < capacity.  (An open-list search: "roots" above.) */
struct NgwSearchRoots {
    const int32_t* roots;       /* [count] */
    const int32_t* where;       /* [count] */
    const int32_t* value;       /* [count] */
    const uint8_t* best;        /* [count] */
    int32_t* parents;           /* [capacity] */
    int32_t* g;                 /* [pool] */
    int32_t* bucket;            /* [pool] */
    int64_t count, capacity, pool;
    /* an open-list search: f != NULL (all NULL / 0 in a closed one) */
    int32_t* f;                 /* [pool] */
    int32_t* h;                 /* [pool] */
    int32_t* slot_of_bucket;    /* [buckets] */
    const int32_t* dist;        /* [count][K]: ngw_snapshot_walk of the roots; NULL: no heuristic */
    const int32_t* weights;     /* [K] */
    int64_t buckets;
    int32_t K, mode;
    const int32_t* recipe;      /* [count]: the recipe term of every root; NULL: none */
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_search_roots_launch(const struct NgwSearchRoots* x, hipStream_t stream);

/* The recipe heuristic (ngw_recipe.inc, ngw_abi_recipe.cpp; the contract is include/ngw.h's ngw_snapshot_recipe_costs): out[j] = the relaxed-plan cost
 * of row idx[j] of `src` (a snapshot or the state slab; a NULL list = j itself) under `prog`, the program as the host unit packs it - items resolved
 * to rule numbers, the flagged map items to count slots:
 *   rule r: d = max(0, need[r] - have), have = inv[out_item] + (map_slot >= 0: the cells equal to map_item[map_slot]); n = ceil(d / out_qty);
 *           h = min(h + n * cost, NGW_VALUE_NONE - 1); need[in_rule[i]] = min(need + n * in_qty[i], 2^31 - 1) for the inputs that have a rule (in_rule
 *           > r, -1: none); n > 0: need[tool_rule] = max(need, 1).  need[goal_rule] starts at 1 (goal_rule -1: h = 0).
 * An index outside [0, rows) is never used as an address: its cost is 0 and - unless it is NGW_IDX_NONE - NGW_F_BAD_INDEX is raised in *flags.  Nothing
 * but out[0 .. count) and the flags word is stored.  The program travels by value in the kernel's argument block (400 bytes).  With n_map == 0 no map
 * byte is read. */
#define NGW_RECIPE_RULES 16
struct NgwRecipeRule {
    int32_t cost;
    uint16_t out_qty;
    uint8_t out_item, n_in;
    int8_t map_slot, tool_rule;     /* -1: none */
    int8_t in_rule[4];              /* -1: the input has no rule */
    uint16_t in_qty[4];
    uint16_t pad;
};
struct NgwRecipeProg {
    int32_t n_rules, goal_rule, n_map;
    uint8_t map_item[4];
    struct NgwRecipeRule rule[NGW_RECIPE_RULES];
};
struct NgwRecipe {
    NgwSnapRows src;
    const int32_t* idx;
    uint32_t* flags;
    int32_t* out;
    int64_t count;
    int32_t rows, S2, K;
    struct NgwRecipeProg prog;
};
#ifdef __cplusplus
extern "C"
#endif
hipError_t ngw_recipe_launch(const struct NgwRecipe* x, hipStream_t stream);

/* Tree-search runs (ngw_tree.inc, ngw_abi_tree.cpp; the contract is include/ngw.h's ngw_tree_run): what the four kernels between a guided playout
 * and the table's insert read and write.  The statistics are [buckets][A] (visits int32, returns int64, rows and priors float32) and [buckets] (the
 * mask words); the recorded arrays of the playout are step-major, row t at t * stride; `touched` is the tree's own, step-major [T][cap].
 *   leaf      one lane per pair j < count: d = depth[j]; 1 <= d < length[j] (and d < n): leaf_keys[j] = keys[d - 1][j], leaf_masks[j] = masks[d][j];
 *             otherwise both 0.  Counts the pairs with length >= 1 and the largest depth into `row`, zero-fills `next_row`.
 *   grow      one lane per pair: w = where_leaf[j] in [0, buckets): mask_words[w] = leaf_masks[j] where that word is not 0 (equal states store equal words).  Counts
 *             fresh[j] != 0 and the refusals (leaf_keys[j] != 0 with w < 0) into `row`.
 *   backup    one lane per pair, j < cap: t from T - 1 down to 0, G += rewards[t][j] for t < n (bootstrap[j] first); for t <= min(d, length - 1), d >=
 *             1: the bucket e = where[t][j] (t < d) or where_leaf[j] (t == d; none without where_leaf) and a = actions[t][j]; e in [0, buckets) and a
 *             in [0, A): visits[e][a] += 1, returns[e][a] += G - integer atomics, combined inside the wave where `combine` is set - and touched[t][j]
 *             = e; -1 everywhere else, also for the lanes count <= j < cap.  Counts the adds into `row`.
 *   reweight  one lane per entry q < n_list of `list`: the bucket e = list[q] in [0, buckets) - unless the lane before it in the wave names the same -
 *             gets its row by the PUCT rule of include/ngw.h.  A bad prior raises NGW_F_BAD_WEIGHT in *flags.
 *   reweight16  the same list, one entry per 16 lanes (lane l holds the actions l, l + 16, l + 32): the row by the spread rule with S = `spread` in
 *             [1, 64] - at S = 1 the bytes of `reweight`; an entry equal to the entry before it in the list is skipped.
 *   backup with g != 65536: G_t = rewards[t][j] + ((g * G_{t+1}) >> 16) for the executed steps t < length, in int64; the steps behind them add as before.
 * No index becomes an address before it is checked against buckets, A, count and cap.  `row` / `next_row` NULL: nothing is counted. */
struct NgwTree {
    int32_t* visits;
    unsigned long long* returns;
    uint64_t* mask_words;
    float* rows;
    const float* priors;            /* NULL: every prior is 1 */
    const int32_t *actions, *rewards, *where, *depth, *length;
    const int32_t* bootstrap;       /* NULL: none */
    const uint64_t *keys, *masks;
    uint64_t *leaf_keys, *leaf_masks;
    int32_t* where_leaf;            /* backup: NULL = no pair has a leaf */
    const uint8_t* fresh;
    int32_t* touched;
    const int32_t* list;
    uint32_t *row, *next_row, *flags;
    int64_t count, cap, stride, buckets, n_list;
    int32_t T, n, A, combine;       /* T: the tree's steps (rows of `touched`); n <= T: the steps of the recorded arrays */
    float c, q_init;
};
/* The rule of ngw_tree_set_rule, a second argument of the two kernels that read it - NgwTree keeps its layout, so the four kernels above compile to the
 * code they were: spread = S of the spread rule (reweight16), g = discount_q16 of the backup (65536: none, the undiscounted kernel runs). */
struct NgwTreeRule { int32_t spread, g; };
#define NGW_TREE_BLOCK 256       /* threads per workgroup: four waves, one entry per lane (reweight16: one entry per 16 lanes) */
#define NGW_TREE_COLS 8          /* uint32 per stats row */
#define NGW_TREE_ALIVE 0
#define NGW_TREE_GROWN 1
#define NGW_TREE_REFUSED 2
#define NGW_TREE_BACKED 3
#define NGW_TREE_DEPTH 4
#ifdef __cplusplus
extern "C" {
#endif
hipError_t ngw_tree_leaf_launch(const struct NgwTree* x, hipStream_t stream);
hipError_t ngw_tree_grow_launch(const struct NgwTree* x, hipStream_t stream);
hipError_t ngw_tree_backup_launch(const struct NgwTree* x, hipStream_t stream);
hipError_t ngw_tree_backup_discount_launch(const struct NgwTree* x, const struct NgwTreeRule* r, hipStream_t stream);
hipError_t ngw_tree_reweight_launch(const struct NgwTree* x, hipStream_t stream);
hipError_t ngw_tree_reweight16_launch(const struct NgwTree* x, const struct NgwTreeRule* r, hipStream_t stream);
#ifdef __cplusplus
}
#endif

#endif
