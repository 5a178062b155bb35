/* ngw.h — C-ABI of the MI355X-native batched step()/reset() hot path of gym-novel-gridworlds.
 *
 * The reference has no FFI of its own: its hot path sits behind the OpenAI-gym `gym.Env`
 * Python API (reference: gym_novel_gridworlds/envs/pogostick_v1_env.py:86 reset, :230 step,
 * :214 get_observation; envs/bow_v1_env.py same lines; novelty_wrappers.py:117-213 AxeMedium,
 * :991-1034 AddItem, :1586 inject_novelty).  This header is the boundary a maintainer would bind
 * from Python with ctypes (stub shown in INTEGRATION.md): plain pointers and sizes only.
 *
 * One handle = N independent environments resident on ONE GPU (one process per GPU; shard by
 * creating one handle per rank with `env_index_base = rank * N`).  All state lives in HBM as
 * structure-of-arrays; the observation buffers ARE the state, updated in place, see DESIGN.md.
 *
 * Every function returns 0 on success or a negative NGW_E_* code; ngw_last_error() gives the
 * thread-local message.  A handle is not thread-safe (one host thread per handle), matching the
 * single-threaded reference.
 */
#ifndef NGW_H
#define NGW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGW_ABI_VERSION 3    /* 3: the narrow wire format carries int32 rewards (ngw_host_step_layout_packed: section 3); the lidar rows default to int32 */

#define NGW_MAX_ITEMS 24        /* reference asserts len(items) <= max_items = 20 (pogostick_v1_env.py:75,220) */
#define NGW_MAX_ACTIONS 48
#define NGW_MAX_RECIPES 8
#define NGW_MAX_RECIPE_INPUTS 4  /* the reference's recipes have <= 3 inputs (pogostick_v1_env.py:56-59) */
#define NGW_MAX_START_ITEMS 8
#define NGW_MAX_INV_START 4
#define NGW_MAX_PASSES 4          /* shuffled-subset reset passes of one stack of wrappers */
#define NGW_MAX_MAP_SIZE 64     /* S; the LDS-resident kernel supports S*S <= 4096 */

/* error codes */
#define NGW_OK 0
#define NGW_E_INVALID_ARG (-1)
#define NGW_E_HIP (-2)           /* a HIP runtime call failed; no CPU fallback exists */
#define NGW_E_INVALID_ACTION (-3)/* reference: ValueError "<a> is not in list" (pogostick_v1_env.py:236) */
#define NGW_E_PLACEMENT (-4)     /* reference: AssertionError "Cannot place items, increase map size!" (:167) */
#define NGW_E_NO_DEVICE (-5)

/* device-side sticky error flags (ngw_error_flags) */
#define NGW_F_INVALID_ACTION 1u
#define NGW_F_PLACEMENT 2u
#define NGW_F_BAD_INDEX 4u      /* ngw_snapshot_save / ngw_snapshot_restore / ngw_snapshot_expand / ngw_snapshot_rollout / ngw_snapshot_playout: an env or slot index outside its range (that copy / pair was skipped); ngw_snapshot_lidar / ngw_snapshot_agent_view / ngw_snapshot_action_mask: a slot index outside its range (that output row is all zeros); ngw_state_keys: a row index outside its range (that key is 0); ngw_snapshot_walk: a row index or an item id outside its range (that row is all -1) */
#define NGW_F_TABLE_FULL 8u     /* ngw_key_table_insert: a key found neither itself nor a free bucket after probing every bucket (it was refused: where = -1, fresh = 0) */
#define NGW_F_BAD_WEIGHT 16u    /* ngw_sample_actions / ngw_snapshot_playout_weighted: a weight that is negative, NaN or above 2^64 (it counted as 0) */
#define NGW_F_FRONTIER_FULL 32u /* ngw_frontier_compact: more flags set than the list has room for (the first `capacity` of them were kept); ngw_frontier_alloc: fewer slots left below the limit than were asked for (the entries behind them are NGW_IDX_NONE) */

/* A pair that is not there.  Every call that gathers rows through an index list in DEVICE memory - ngw_snapshot_save / _restore / _copy / _expand /
 * _rollout* / _playout*, ngw_snapshot_lidar / _agent_view / _action_mask, ngw_state_keys, ngw_successor_keys, ngw_sample_actions, ngw_snapshot_walk - skips
 * pair j when ANY of its indices (the source row, the destination row, the walk's item) is NGW_IDX_NONE: it stores for that pair exactly what it stores
 * for a pair with an index out of range - nothing, zeros, action -1, key 0, distance -1, as the call says - and does NOT raise NGW_F_BAD_INDEX.  Every
 * other value outside the range (-1, the row count, 2^31 - 1, ...) raises the flag as before.  It is how a list of fixed capacity carries fewer
 * pairs than it has entries: ngw_frontier_compact and ngw_frontier_alloc pad their lists with it.  Key 0 is what a skipped pair's key reads, and key 0
 * is never stored by ngw_key_table_insert (where = -1, fresh = 0, no flag): a padded list goes through keys -> insert with no special case.
 * Lists checked on the host are not device lists: their range check stands. */
#define NGW_IDX_NONE INT32_MIN

/* action kinds (act_kind[]); act_arg[] = recipe index (CRAFT) or item id (SELECT) */
enum { NGW_ACT_FORWARD = 0, NGW_ACT_LEFT = 1, NGW_ACT_RIGHT = 2, NGW_ACT_BREAK = 3, NGW_ACT_PLACE = 4,
       NGW_ACT_EXTRACT = 5, NGW_ACT_CRAFT = 6, NGW_ACT_SELECT = 7,
       NGW_ACT_CHOP = 8 /* AddChopAction, novelty_wrappers.py:1267 */, NGW_ACT_JUMP = 9 /* AddJumpAction, :1340 */ };

/* info['message'] codes; the host formats the string (reference strings cited in spec.py) */
enum { NGW_XF_FIRE_SKIP_BREAK = 1, NGW_XF_CRATE_IN_FENCE = 2 };
enum { NGW_PASS_ADDITEM = 1, NGW_PASS_REPLACE = 2, NGW_PASS_FENCE = 3 };   /* ngw_spec.pass_kind */
/* passes sampled without an index array (see ngw_spec.n_passes): AddItem / Crate (air of the interior), ReplaceItem / FireWall of the wall ring */
#define NGW_PASS_SPARSE(kind, from, wall_item) ((kind) == NGW_PASS_ADDITEM || ((kind) == NGW_PASS_REPLACE && (from) == (wall_item)))
#define NGW_PASS_MARK 0x7F       /* transient cell value while such a pass runs (item ids are < NGW_MAX_ITEMS) */
enum { NGW_MSG_NONE = 0, NGW_MSG_BLOCK_IN_PATH = 1, NGW_MSG_CANNOT_BREAK = 2 /* arg = item */,
       NGW_MSG_PLACED = 3 /* arg = item */, NGW_MSG_ALREADY_EXISTS = 4 /* arg = front item */,
       NGW_MSG_NOT_IN_INVENTORY = 5, NGW_MSG_EXTRACT_NO_SRC = 6, NGW_MSG_EXTRACT_NOT_NEAR = 7,
       NGW_MSG_MISSING_ITEMS = 8 /* arg = recipe<<8 | mask over the recipe's inputs in dict order */,
       NGW_MSG_NEED_TABLE = 9, NGW_MSG_CRAFTED = 10 /* arg = crafted item */,
       NGW_MSG_NEED_AXE = 11 /* arg = axe item: "Cannot break without <axe> selected" */,
       NGW_MSG_CANNOT_CHOP = 12 /* arg = item */,
       NGW_MSG_FENCE_RESTRICTION = 13 /* "Cannot break due to fence restriction" */,
       NGW_MSG_FIRE_WALL = 14 /* "You died due to fire_wall" */ };

/* packed per-env info word produced by the step kernel:
 *   bit 0 result | bit 1 done | bits 2..7 cost code | bits 8..15 message code | bits 16..31 message arg */
#define NGW_INFO_RESULT(w) ((w) & 1u)
#define NGW_INFO_DONE(w) (((w) >> 1) & 1u)
#define NGW_INFO_COST(w) (((w) >> 2) & 63u)
#define NGW_INFO_MSG(w) (((w) >> 8) & 255u)
#define NGW_INFO_ARG(w) ((w) >> 16)

/* Immutable environment specification, compiled on the host from (env id, map_size, novelty args)
 * into flat integer look-up tables (SURVEY.md §8(a) a2 "LUT set").  `cost_*` fields are CODES into
 * the host-side step_cost table (the reference mixes Python float and int step costs,
 * pogostick_v1_env.py:257-470; 27.906975 is not float32-representable, so values never enter the GPU). */
typedef struct ngw_spec {
    int32_t abi_version;                 /* = NGW_ABI_VERSION */
    int32_t map_size;                    /* S  (pogostick_v1_env.py:30) */
    int32_t n_items;                     /* K  incl. air(0) and wall (set_items_id :200-212) */
    int32_t n_actions;                   /* A = len(actions_id) (:52-68); may exceed action_space.n with novelties */
    int32_t n_recipes;                   /* R */
    int32_t reward_step;                 /* -1  (:239) */
    int32_t reward_done;                 /* 50  (:82, forced while inv[goal] >= 1, :354-357) */
    uint8_t act_kind[NGW_MAX_ACTIONS];
    uint8_t act_arg[NGW_MAX_ACTIONS];
    uint8_t breakable[NGW_MAX_ITEMS];    /* item not in unbreakable_items (:41,:283) */
    uint8_t entity[NGW_MAX_ITEMS];       /* item in entities, picked up by grab_entities (:538-554) */
    int8_t break_reward[NGW_MAX_ITEMS];  /* +10 for tree_log else -1 (:288-289); BreakIncrease: +10 for every block */
    uint8_t break_qty[NGW_MAX_ITEMS];    /* blocks gained by Break without an axe: 1, or 2 (BreakIncrease, novelty_wrappers.py:1449-1454) */
    uint8_t wall_item, table_item, goal_item, n_entities;
    /* recipes (:56-59, craft :413-474) */
    uint8_t recipe_in[NGW_MAX_RECIPES][NGW_MAX_ITEMS];        /* required quantity per item id */
    uint8_t recipe_n_in[NGW_MAX_RECIPES];
    uint8_t recipe_in_item[NGW_MAX_RECIPES][NGW_MAX_RECIPE_INPUTS]; /* inputs in dict order (message order) */
    uint8_t recipe_out_item[NGW_MAX_RECIPES];
    uint8_t recipe_out_qty[NGW_MAX_RECIPES];
    uint8_t recipe_needs_table[NGW_MAX_RECIPES];             /* len(input) > 1 (:444) */
    uint8_t cost_missing[NGW_MAX_RECIPES], cost_no_table[NGW_MAX_RECIPES], cost_ok[NGW_MAX_RECIPES];
    /* reward of a successful craft: 10 Pogostick-v1 (:455) / 50 Bow-v1 (bow_v1_env.py:424); the craftable axe of
     * AxeHard / AxetoBreakHard always gives 10 (the wrappers' own craft(), novelty_wrappers.py:331) */
    int8_t recipe_reward[NGW_MAX_RECIPES];
    /* fixed-action cost codes */
    uint8_t cost_forward, cost_turn, cost_break, cost_place, cost_extract, cost_select;
    uint8_t cost_chop, cost_jump;        /* 3600.0 * 1.2 (novelty_wrappers.py:1294), 27.906975 * 2 (:1381) */
    int8_t chop_reward;                  /* reward_intermediate for any breakable block (:1303) */
    uint8_t _pad3;
    /* Place_<item> (:295-314): place `place_item` in front; +place_reward iff a 4-neighbour of the front cell is place_near */
    uint8_t place_item, place_near;
    int8_t place_reward;
    /* Extract_* (Pogostick :315-331, Bow bow_v1_env.py:293-304) */
    uint8_t ext_src, ext_near /* 0 = no adjacency requirement */, ext_out, ext_qty, ext_consume, ext_cost_ok;
    int8_t ext_reward;
    /* Break override of the axe novelties (novelty_wrappers.py:144-183); axe_item = 0 -> base Break */
    uint8_t axe_item, axe_cost, axe_qty;
    int8_t axe_reward;
    uint8_t axe_required;                /* AxetoBreak*: Break fails without the selected axe (novelty_wrappers.py:589-591) */
    uint8_t _pad2[3];
    /* reset (:86-157): items placed in insertion order of items_quantity */
    uint8_t n_start;
    uint8_t start_item[NGW_MAX_START_ITEMS];
    uint8_t start_qty[NGW_MAX_START_ITEMS];
    /* Pogostick-v0 reset pass (pogostick_v0_env.py:156-178): put one `tap_item` on a free 4-neighbour (random direction)
     * of a random `tap_near` block; tap_item = 0 -> disabled */
    uint8_t tap_item, tap_near;
    /* items present in the inventory after every reset: AxeEasy / AxetoBreakEasy (novelty_wrappers.py:29-35, :456-462: the
     * axe), AxetoBreakHard (:663-672: the axe's ingredients) */
    uint8_t n_inv_start;
    uint8_t inv_start_item[NGW_MAX_INV_START], inv_start_qty[NGW_MAX_INV_START];
    /* Shuffled-subset reset passes, in the order they run = the order their wrappers were injected (a wrapper's reset() calls
     * the wrapped env's first): np.where(<predicate>) row-major, np.random.shuffle, randint(pct_lo, pct_hi), then the first
     * ceil(len * pct / 100) cells are edited (never the agent cell).  pass_kind: NGW_PASS_ADDITEM - AddItem / Crate
     * (novelty_wrappers.py:1013-1034, :1071): air cells become pass_item; NGW_PASS_REPLACE - ReplaceItem / FireWall
     * (:1129-1148): cells holding pass_from become pass_item; NGW_PASS_FENCE - Fence / FenceRestriction (:867-889): every free
     * 8-neighbour of a chosen non-air, non-wall cell gets pass_item (add_fence_around, pogostick_v1_env.py:524-536).  Any
     * number of passes of the same kind may be stacked (additem + crate, fence + fencerestriction, replaceitem + firewall).
     *
     * How the subset is DRAWN on the device (per-(env, episode) Philox stream; the CPU oracle's Philox mode runs the same
     * steps, its MT19937 mode follows numpy call for call): passes whose source cells are the air of the interior or the
     * wall of the ring (NGW_PASS_SPARSE) never build the index array.  The result of shuffle + "first cnt" is a uniformly
     * random cnt-subset of the matching cells - the order inside it is irrelevant, every chosen cell gets the same item -
     * and that is what is sampled: percent first (the numpy bounded draw, as before), cnt = ceil(len * pct / 100), then
     * min(cnt, len - cnt) distinct matching cells by rejection (the complement when that is the smaller set).  A candidate
     * is a cell index of nb = bit_length(S*S - 1) bits: field j of word k of a Philox block (32 / nb fields per word, from
     * the low end), taken in the order j = 0: words 0..3, j = 1: words 0..3, ...; blocks start at the next block boundary
     * and the rest of the last one is discarded; a candidate beyond the map, not matching or already taken is skipped.
     * Same distribution of maps as the reference's, pinned by the distribution fixtures tests/golden/g6_*.npz; every other
     * pass keeps shuffle-then-prefix. */
    uint8_t n_passes;
    uint8_t pass_kind[NGW_MAX_PASSES], pass_item[NGW_MAX_PASSES], pass_from[NGW_MAX_PASSES];
    uint8_t pass_pct_lo[NGW_MAX_PASSES], pass_pct_hi[NGW_MAX_PASSES];
    /* FenceRestriction Break predicate (:906-988) on fence_item: fence_mode 0 none (fence, fencerestriction easy), 1 medium (no
     * fence beside the AGENT, across its facing), 2 hard (no fence in the 3x3 around the block in front) */
    uint8_t fence_item, fence_mode;
    /* FireWall.step (:1164-1200): after the step, a fire_item 4-neighbour of the agent -> reward fire_reward, done,
     * message 'You died due to fire_wall'; fire_item = 0 -> disabled */
    uint8_t fire_item;
    int8_t fire_reward;
    /* Crate.step (:1078-1092): Break with crate_item in front first adds crate_add[item] of every item to the
     * inventory (the ingredient multiset drawn at injection, :1055-1068); crate_item = 0 -> disabled */
    uint8_t crate_item;
    uint8_t crate_add[NGW_MAX_ITEMS];
    /* wrapper nesting of a stack, as far as the step can tell: NGW_XF_FIRE_SKIP_BREAK - the FireWall wrapper sits BELOW a
     * Break-overriding one (axe / axetobreak / breakincrease handle Break without calling the env they wrap), so its check
     * does not run on Break steps; fire_skip_recipe = 1 + recipe of a craftable axe whose wrapper sits above FireWall (its
     * Craft action is handled the same way); NGW_XF_CRATE_IN_FENCE - the Crate wrapper sits below FenceRestriction, so a
     * restricted Break never reaches it */
    uint8_t ext_flags, fire_skip_recipe;
} ngw_spec;

/* LidarInFront observation (reference gym_novel_gridworlds/observation_wrappers.py:10-80): `num_beams` rays at equally
 * spaced angles around the agent; per ray, the distance to the first non-air block, reported in the channel of that
 * block's item (0 if the block is not a lidar item or nothing is hit within max_range), followed by the inventory of
 * the breakable items in alphabetical order.  The host precomputes the integer ray offsets with the reference's own
 * float arithmetic (np.round(np.cos(angle), 2), np.round(range * ratio)), so the GPU only marches integers. */
#define NGW_LIDAR_MAX_BEAMS 16
#define NGW_LIDAR_MAX_RANGE 64
typedef struct ngw_lidar_cfg {
    int32_t num_beams;                   /* LidarInFront(env, num_beams) */
    int32_t max_range;                   /* int(sqrt(2 * (map_size - 2)^2)) at wrap time (observation_wrappers.py:25) */
    int32_t n_chan;                      /* len(lidar_items) = items without air and the goal item (:21-24) */
    int32_t n_inv;                       /* inventory entries appended (:74-75) */
    uint8_t chan_of_item[NGW_MAX_ITEMS]; /* 1-based lidar channel of an item id, 0 = not a lidar item */
    uint8_t inv_item[NGW_MAX_ITEMS];     /* item ids of the appended inventory, in sorted-name order */
    int8_t dr[4][NGW_LIDAR_MAX_BEAMS][NGW_LIDAR_MAX_RANGE];   /* [facing][beam][range-1] row offset */
    int8_t dc[4][NGW_LIDAR_MAX_BEAMS][NGW_LIDAR_MAX_RANGE];   /* column offset */
} ngw_lidar_cfg;

typedef struct ngw_handle ngw_handle;

int ngw_abi_version(void);
int ngw_spec_size(void);            /* sizeof(ngw_spec), checked by the host binding */
const char* ngw_last_error(void);
/* Number of visible GPUs (hipGetDeviceCount); 0 when there is none. */
int ngw_device_count(void);

/* Creates n_envs environments on GPU `device`.  `seed` keys the per-env counter-based reset streams
 * (Philox4x32-10, counter = (word block, episode, global env index)); `env_index_base` is the global index
 * of local env 0 so results do not depend on how envs are sharded over GPUs.  Replaces
 * `gym.make(id)` + attribute edits + `inject_novelty` (gym_novel_gridworlds/__init__.py:57-60). State is
 * undefined until ngw_reset / ngw_set_state. */
int ngw_create(const ngw_spec* spec, int64_t n_envs, int device, uint64_t seed, int64_t env_index_base,
               ngw_handle** out);
int ngw_destroy(ngw_handle* h);

/* autoreset = 0 reproduces the reference (sticky done, no time limit).  autoreset = 1 (classic gym.vector
 * "same-step" form): every call steps every env; an env whose step ended with done, or whose step_count
 * reached `horizon` (> 0), is reset in the same call and the observation returned is the new episode's first
 * one; reward/info are the terminal step's, done = 1 for both endings (info bit 1 set only for goal-done). */
int ngw_set_autoreset(ngw_handle* h, int autoreset, int horizon);
/* Run the handle's kernels on an external hipStream_t (e.g. torch's current stream); NULL = own stream. */
/* Prepared next episodes.  A reset (explicit, or the same-step autoreset) normally runs the reference's placement loop
 * (~40 dependent random draws per env) inside the step launch; when only a few envs of a batch end in a given step, the
 * whole launch waits for them.  With every_n_steps > 0 the library keeps, per env, the first state of its NEXT episode
 * in shadow buffers: a reset then copies that row (one memory round trip), and one extra launch every `every_n_steps`
 * batched steps (and after every ngw_reset) re-prepares the rows consumed since.  Results are bit-identical with the
 * feature on or off (the shadow row is the output of the same per-(env, episode) Philox stream).  0 = off.
 * ngw_set_autoreset(h, 1, horizon) switches it ON by itself (a refill every 3/4 horizon, 32 to 128 steps, 32 without a horizon; not for horizons under 64 steps, where
 * rows would go stale before they are needed) unless the caller has chosen a cadence with this call, before or after.
 * Fused rollouts run as launches of at most every_n_steps steps with the refills between them. */
int ngw_set_reset_prefetch(ngw_handle* h, int32_t every_n_steps);
/* The refill cadence in effect (0 = prepared episodes off): what ngw_set_reset_prefetch set, or the default ngw_set_autoreset chose. */
int ngw_get_reset_prefetch(ngw_handle* h, int32_t* every_n_steps);
/* How many episodes ahead are prepared per env: depth 1, 2, 4 or 8 (a power of two; shadow memory grows with it), 0 = automatic
 * (the default: 1, growing to 2 and 4 by itself when envs end episodes faster than a refill comes round - FireWall kills within
 * a few steps - so that a reset still finds a prepared row; see adapt_cadence in ngw_abi.cpp).  Results do not depend on it. */
int ngw_set_reset_prefetch_depth(ngw_handle* h, int32_t depth);
int ngw_get_reset_prefetch_depth(ngw_handle* h, int32_t* depth);
int ngw_set_stream(ngw_handle* h, void* hip_stream);
/* Order the handle's stream and another hipStream_t of the same device behind each other WITHOUT a host wait (one event
 * record + one stream wait): handle_waits != 0 - work submitted to the handle after this call runs after everything
 * `other_stream` holds now; handle_waits == 0 - the other way round.  What dist.py uses around the one collective (pack /
 * unpack launches on the handle's stream, RCCL on torch's current stream); NULL = the default stream. */
int ngw_stream_order(ngw_handle* h, void* other_stream, int handle_waits);

/* reset(): pogostick_v1_env.py:86-157 (+ AddItem.reset).  mask = NULL resets all envs, else mask[i] != 0. */
int ngw_reset(ngw_handle* h, const uint8_t* mask_host);
/* ngw_reset + the state it produced, in ONE call (any output may be NULL): what reset() of the host API returns.  For handles of at
 * most one wavefront (the single-env gym.Env adapter) it waits for the reset kernel alone - not for the refill launch that
 * re-prepares the consumed episode behind it - by polling a word the kernel writes when its stores (the state in HBM and its
 * host mirror, see ngw_obs_device_ptrs) are out. */
int ngw_reset_host(ngw_handle* h, const uint8_t* mask_host, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv, uint8_t* selected,
                   int32_t* step_count, uint32_t* error_flags);
/* step(action_id): pogostick_v1_env.py:230-367 / AxeMedium.step.  Host actions are validated first
 * (NGW_E_INVALID_ACTION, nothing stepped - the reference raises before touching state). */
int ngw_step(ngw_handle* h, const int32_t* actions_host);
/* Same with actions already in HBM; an out-of-range id sets NGW_F_INVALID_ACTION and leaves that env untouched. */
int ngw_step_device(ngw_handle* h, const int32_t* actions_dev);
/* n_steps consecutive ngw_step_device launches from ONE call: step i reads actions_dev + i * step_stride (int32 elements).  For
 * short open-loop stretches where a host loop's per-call overhead (an interpreter, a binding) would outweigh the 4-5 us a step
 * takes on the device; semantically identical to n_steps calls of ngw_step_device. */
int ngw_step_device_many(ngw_handle* h, const int32_t* actions_dev, int64_t step_stride, int32_t n_steps);
/* ngw_step + ngw_get_obs + ngw_get_step_out as ONE call with one stream synchronisation: what a host-driven loop pays per
 * step() is launch and PCIe latency, so the three round trips of the separate calls matter at small batch sizes.  Any
 * output pointer may be NULL; batches whose outputs fit in 1 MiB travel through host memory the GPU addresses directly
 * (no copy calls at all); page-locked buffers (ngw_host_alloc) make the copies truly asynchronous. */
int ngw_step_host(ngw_handle* h, const int32_t* actions_host, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv,
                  int32_t* reward, uint8_t* done, uint8_t* result, uint8_t* cost_code, uint16_t* msg_code, uint16_t* msg_arg,
                  uint32_t* error_flags /* the sticky NGW_F_* word, as ngw_error_flags */,
                  uint8_t* selected /* item id, 0 = '' */, int32_t* step_count);
/* Big batches: when the output arrays handed to ngw_step_host are the sections of ONE page-locked block laid out as this call
 * says (offsets11[0..9] = byte offsets of map | agent_location | agent_facing_id | inventory | reward | done | info words
 * (internal) | error flags | selected | step_count from the block's start, each section padded to 256 bytes - in memory the
 * sections lie in the order map, inventory, selected, then the rest; offsets11[10] = block size; allocate it with
 * ngw_host_alloc) AND the caller hands in the same block call after call (it is his mirror of the observation), a step moves
 * only what changed: the pose / reward / done / info / step_count sections with ONE copy (26 B per env), and of the map,
 * inventory and selected rows only the 16-byte pieces that differ from what the block already holds - the device keeps a
 * shadow of the block's content and writes the differing pieces straight into it across PCIe.  The first call on a block, and
 * the first one after anything else touched the state (ngw_reset, ngw_set_state, device steps, rollouts, graph replays) or
 * after ngw_host_mirror_invalidate, copies the whole observation; NGW_HOST_DELTA=0 in the environment makes every call do so.
 * The block must not be written by the caller between calls. */
int ngw_host_step_layout(ngw_handle* h, uint64_t* offsets11);
/* The next ngw_step_host copies the whole observation again (e.g. after the caller wrote into his block). */
int ngw_host_mirror_invalidate(ngw_handle* h);
/* Fused bench mode: T steps in one launch with on-device uniform actions
 * a(t, env) = (word (t & 3) of philox(action_seed; t >> 2, env) * A) >> 32; state stays in LDS/registers between
 * steps and every step's changes are written through to the observation buffers. */
int ngw_rollout(ngw_handle* h, int32_t n_steps, uint64_t action_seed, int64_t t0);
/* The same fused launch driven by the CALLER's actions (open-loop sequences, action repeat / frame skip, evaluating plans):
 * batched step t takes int32 actions_dev[t * step_stride + e] (device memory, step_stride >= n_envs).  An action outside
 * [0, n_actions) leaves that env untouched for that step and raises NGW_F_INVALID_ACTION, as in ngw_step_device. */
int ngw_rollout_actions(ngw_handle* h, const int32_t* actions_dev, int64_t step_stride, int32_t n_steps);

/* Per-step outputs of the fused rollouts, for whoever consumes them (the reference's loop sees (obs, reward, done, info) after
 * every step: tests/random_action.py:51-64, tests/train.py:122-135).  With rows set, step t of a ngw_rollout /
 * ngw_rollout_actions call also stores reward_rows_dev[t * row_stride + e] (int32) and done_rows_dev[t * row_stride + e]
 * (uint8: 1 where the step ended an episode - done, or the horizon under autoreset); either pointer may be NULL, both NULL
 * switches the rows off.  accumulate = 1 additionally keeps four per-env int32 counters across rollout calls: return and
 * length of the running episode, sum of returns and number of the episodes finished so far (ngw_episode_stats reads them
 * into host arrays, any of which may be NULL; clear = 1 zeroes them afterwards).  Device memory, row_stride >= n_envs. */
int ngw_rollout_outputs(ngw_handle* h, int32_t* reward_rows_dev, uint8_t* done_rows_dev, int64_t row_stride, int accumulate);
int ngw_episode_stats(ngw_handle* h, int32_t* run_return, int32_t* run_length, int32_t* sum_return, int32_t* n_episodes, int clear);

/* get_observation(): pogostick_v1_env.py:214-228, batched: map i8 [N,S,S], agent_location i32 [N,2] (r,c),
 * agent_facing_id i32 [N], inventory_items_quantity i32 [N,K] in items_id order.  Any pointer may be NULL. */
int ngw_get_obs(ngw_handle* h, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv);
/* (reward, done, info) of the last step: pogostick_v1_env.py:354-367. */
int ngw_get_step_out(ngw_handle* h, int32_t* reward, uint8_t* done, uint8_t* result, uint8_t* cost_code,
                     uint16_t* msg_code, uint16_t* msg_arg);
/* Full state of envs [first, first+count): the observation arrays plus selected item id (0 = ''),
 * step_count and episode counter.  Checkpoint/restore and oracle-state injection
 * (reference: direct attribute mutation, tests/keyboard_interface.py:93-100). */
int ngw_get_state(ngw_handle* h, int64_t first, int64_t count, int8_t* map, int32_t* loc, int32_t* facing,
                  int32_t* inv, int32_t* selected, int32_t* step_count, uint32_t* episode);
int ngw_set_state(ngw_handle* h, int64_t first, int64_t count, const int8_t* map, const int32_t* loc,
                  const int32_t* facing, const int32_t* inv, const int32_t* selected,
                  const int32_t* step_count, const uint32_t* episode);

/* Page-locked host memory for the arrays handed to ngw_step / ngw_get_obs / ngw_get_step_out: copies to and from
 * pinned buffers run at full PCIe rate without a staging pass (API mode).  Plain malloc'ed arrays work too. */
void* ngw_host_alloc(uint64_t bytes);
int ngw_host_free(void* p);

/* Device pointers of the observation / output buffers (fixed for the handle's lifetime; contents are the state
 * after the last enqueued step and are updated in place by the next one): HBM for every handle.  Handles of at most one
 * wavefront (<= 64 envs: the single-env gym.Env adapter) additionally keep a MIRROR of these rows in page-locked host memory
 * the GPU addresses directly: a step issued by ngw_step_host (an explicit reset by ngw_reset_host) ends by copying the wave's
 * rows there and writing a sequence word the host polls, so such a call is one launch with no copy call and no stream
 * synchronisation. */
int ngw_obs_device_ptrs(ngw_handle* h, void** map, void** loc, void** facing, void** inv);
int ngw_out_device_ptrs(ngw_handle* h, void** reward, void** done, void** info);
int ngw_sync(ngw_handle* h);
/* Reads and clears the sticky device error flags (NGW_F_*). */
int ngw_error_flags(ngw_handle* h, uint32_t* flags);
/* Device time of everything enqueued on the handle's stream between the two calls, measured with a HIP event pair
 * recorded on that stream (bench.py roofline leg: elapsed / launches = average launch duration incl. gaps). */
int ngw_timing_begin(ngw_handle* h);
int ngw_timing_end(ngw_handle* h, double* elapsed_ms);
/* Records the closing event now, without waiting: a later ngw_timing_end only waits for it and reads the pair (a caller that
 * synchronises anyway - a benchmark's closing fence - keeps the event wait out of its wall-clock region). */
int ngw_timing_mark(ngw_handle* h);

/* hipGraph stepping for launch-bound loops: captures n_steps consecutive ngw_step_device launches whose
 * actions are read from actions_dev + i * step_stride (int32 elements) into one executable graph, then replays it.
 * Semantically identical to calling ngw_step_device n_steps * reps times with those action rows.  Prepared next episodes: a graph
 * that is at least half the refill cadence long carries its refills (every replay ends with one, so that it leaves the cadence where
 * it found it); a shorter one is captured without any and ngw_graph_launch issues them between the replays, whenever the next replay
 * would overrun the cadence. */
int ngw_graph_build(ngw_handle* h, const int32_t* actions_dev, int64_t step_stride, int32_t n_steps);
int ngw_graph_launch(ngw_handle* h, int32_t reps);

/* Multi-GPU observation stack (the only collective of the path, outside step()).  One process per GPU,
 * each with its own handle; per step (or whenever the host wants the whole batch) every rank packs its observation and
 * step outputs into ONE contiguous device payload, the ranks gather the payloads on a root (RCCL gather over xGMI through
 * torch.distributed) and the root scatters them into global arrays.
 *   ngw_pack_layout  byte offsets of the seven sections (map i8 [n][S*S] | agent_location i32 [n][2] | agent_facing_id i32 [n] |
 *                    inventory i32 [n][K] | reward i32 [n] | done u8 [n] | info u32 [n]; each padded to 16 bytes) and, in
 *                    offsets8[7], the payload size.  Equal for every rank that holds the same number of envs.
 *   ngw_pack_obs     one kernel launch on the handle's stream: the seven SoA arrays -> payload_dev (16-byte aligned).
 *   ngw_unpack_obs   root side: `world` payloads back to back at payloads_dev -> global arrays (rank r's envs at [r*n, (r+1)*n));
 *                    any destination may be NULL.  One launch on the handle's stream. */
int ngw_pack_layout(ngw_handle* h, uint64_t* offsets8);
int ngw_pack_obs(ngw_handle* h, void* payload_dev);
int ngw_unpack_obs(ngw_handle* h, const void* payloads_dev, int32_t world, int8_t* map, int32_t* loc, int32_t* facing,
                   int32_t* inv, int32_t* reward, uint8_t* done, uint32_t* info);

/* The host step in its NARROW WIRE FORMAT (big batches; what VecNovelGridworld.step() uses from a few thousand envs on).  One
 * page-locked block holds everything a step returns; ngw_host_step_layout_packed gives its section offsets (index: 0 map int8
 * [n][S*S], 1 inventory int32 [n][K], 2 pose uint32 [n] = r | c << 8 | facing << 16 | selected << 24, 3 reward int32 [n] (ABI 3: the
 * type ngw_step_host returns whatever the batch size; int16 before), 4 done uint8 [n], 5 info uint32 [n] (NGW_INFO_*), 6 error flags
 * uint32 followed by one uint32 the library uses itself (the sequence number of the last finished step: the call polls it instead of
 * synchronising the stream); sections padded to 256 bytes, offsets8[7] = the block's size).
 * ngw_step_host_packed(h, actions, block, with_map): int32 actions from host memory are validated and narrowed to bytes on the way
 * into a buffer the step kernel reads in place (no copy call); map and inventory are refreshed by deltas as in ngw_step_host (the block
 * is a mirror the caller hands in call after call; with_map = 0 skips the map's delta for this call); the dense sections 2-6 - 13 B per
 * env instead of the 26 B of the int32 arrays - are stored straight into the block by the device once the block is a mirror (mapped
 * into the GPU's address space; the first call on a block, and a block that cannot be mapped, bring them across with one copy).
 * In that steady state the call is ONE launch: the step kernel itself stores what the step changes into the block (system-scope
 * stores) - cells, inventory slots, the rows of envs that start an episode, the dense sections, and the fused lidar rows when
 * ngw_lidar_host_rows registered a buffer and n_envs is a multiple of 64 - and the call returns when the kernel's last block has
 * published its sequence number; a refill launch behind the step may still be running then (it touches nothing the caller sees).
 * Widening (pose bytes -> int32 arrays) is the caller's, when he needs it. */
int ngw_host_step_layout_packed(ngw_handle* h, uint64_t* offsets8);
int ngw_step_host_packed(ngw_handle* h, const int32_t* actions_host, void* block, int with_map);

/* Terminal observations under same-step autoreset.  A step that ends an env's episode (done, or the horizon) returns the NEXT
 * episode's first observation (ngw_set_autoreset); the reference's loops look at the last observation of the old one before they
 * reset (tests/test.py:30-41, enjoy.py:107-116), and a learner bootstraps from it at a horizon cut.  enable = 1: the envs that reset in
 * a step launch first copy the state their episode ended in - map row, pose, inventory row - into a side set, which
 * ngw_get_terminal_obs copies out whole ([n_envs] rows; row e is meaningful for the envs whose `done` the last step set, and keeps its
 * value until env e ends an episode again) and ngw_terminal_device_ptrs exposes in place.  Off by default; when off the step kernels'
 * hot path is untouched (the copy sits behind the "some lane resets" branch).  Fused rollouts capture too: the lane that resets inside
 * the T-loop stores its map and inventory row from LDS into the side set first; after a rollout row e holds the state env e's LAST
 * finished episode ended in (the per-step done rows of ngw_rollout_outputs say which steps ended one). */
int ngw_set_terminal_capture(ngw_handle* h, int enable);
int ngw_get_terminal_obs(ngw_handle* h, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv);
int ngw_terminal_device_ptrs(ngw_handle* h, void** map, void** loc, void** facing, void** inv);

/* Which per-launch step kernel this handle's ngw_step* calls run right now: *map_in_place = 1 - the one that reads the <= 14 map
 * cells a step needs straight from HBM (the default at every map size), 0 - the one that stages the wave's 64 maps through
 * LDS (any size while the fused lidar epilogue is on, or where NGW_NOSTAGE says so).  What bench.py names its kernel from.
 * The word carries two more flags, so test it with `& 1`, not `== 1`.  Flag 2 - batched steps that bring an int32 action row run the in-place kernel's instantiation for the plain
 * spec class (at most 12 items, no Jump action, no entities, both "near" rules on one item, no wrapper predicates, nothing fused, every
 * array within 4 GB of its base; NGW_STEP_PLAIN=0 switches it off); flag 4 - the last per-launch step, or the launches the current graph
 * captured, ran it (byte and one-env actions, host write-through and the host API's steps, which report a sequence number, never do). */
int ngw_step_kernel_info(ngw_handle* h, int32_t* map_in_place);

/* LidarInFront: configure once, then ngw_lidar() computes the observation of the CURRENT state of every env into a device
 * buffer of [N] rows of num_beams * n_chan beam entries + n_inv inventory entries (enqueued on the handle's stream, after the
 * steps before it). */
int ngw_lidar_configure(ngw_handle* h, const ngw_lidar_cfg* cfg);
int ngw_lidar(ngw_handle* h);
/* enable = 1: every following reset / step / rollout launch also refreshes the lidar observation in its epilogue (the maps are
 * already in LDS there), so ngw_lidar() is not needed; 0 restores the plain kernels.  A fused rollout refreshes it ONCE, for
 * the state the launch ends in (the buffer holds one row per env). */
int ngw_lidar_fuse(ngw_handle* h, int enable);
/* Row format of the observation in the device buffer (and of what ngw_get_lidar copies out):
 *   32 (default)  int32 [len]: what a caller that never calls this function reads (ngw_get_lidar / ngw_lidar_device_ptr);
 *   16            int16 [len]: half the bytes; values saturate at 32767 - a beam entry is a range <= 64, the inventory tail is the
 *                 only part that could ever exceed it;
 *    8            packed: uint8 [num_beams * n_chan] beam entries, padded to an even count, then int16 [n_inv] inventory
 *                 (saturating) - 70 B per env for the reference's 8 beams on Pogostick-v1 against 252 B as int32.
 * ngw_lidar_row_layout reports bytes per row, bytes per beam entry, the byte offset of the inventory tail and bytes per
 * inventory entry of the current format (any pointer may be NULL). */
int ngw_lidar_set_output(ngw_handle* h, int bits);
int ngw_lidar_row_layout(ngw_handle* h, int32_t* row_bytes, int32_t* beam_bytes, int32_t* inv_offset, int32_t* inv_bytes);
int ngw_get_lidar(ngw_handle* h, void* out_host /* [n_envs] rows of the current format */);
/* With the observation fused (ngw_lidar_fuse): rows_host != NULL - a page-locked buffer (ngw_host_alloc) of [n_envs] rows of the current
 * format - makes every following ngw_step_host_packed deliver the rows of the state it produced into that buffer as part of the call
 * (pipelined with the step's slices on big batches: what LidarInFront(VecNovelGridworld).step() returns needs no second call and no
 * second synchronisation); NULL switches it off.  ngw_lidar_set_output / ngw_lidar_configure switch it off too (the row size changed). */
int ngw_lidar_host_rows(ngw_handle* h, void* rows_host);
int ngw_lidar_device_ptr(ngw_handle* h, void** out);

/* AgentMap (observation_wrappers.py:83-129): ngw_agent_view() gathers, for every env, the (2*view_size+1)^2 window of the
 * CURRENT map centred on the agent (0 outside the map; get_agentView :104-121) into an internal int8
 * [n_envs][2*view_size+1][2*view_size+1] buffer.  The reference fixes view_size = 5 (:96).  The other two entries of that
 * wrapper's observation (agent_facing_id, inventory_items_quantity) are the ngw_get_obs buffers. */
int ngw_agent_view(ngw_handle* h, int view_size);
int ngw_get_agent_view(ngw_handle* h, int8_t* out_host);
int ngw_agent_view_device_ptr(ngw_handle* h, void** out);
/* The AgentMap window kept current.  ngw_agent_view_fuse(h, view_size, on) with on != 0 allocates the buffer of ngw_agent_view(h, view_size), fills
 * it for the current state, and from then on every committed step and every reset - ngw_step, ngw_step_device, ngw_step_device_many, ngw_step_host,
 * ngw_step_host_packed, a replayed graph (ngw_graph_launch: the state the last captured step leaves), the fused rollouts, ngw_reset and
 * ngw_reset_host with or without a mask - leaves in it, on the handle's stream, the windows of the state the call produced: byte for byte what
 * ngw_agent_view(h, view_size) issued right behind that call would gather.  For an env whose step ended its episode under autoreset that is the new
 * episode's first state, as in every other observation.  ngw_agent_view_device_ptr returns the buffer; it stays the same allocation until the
 * next ngw_agent_view_fuse.
 *   on = 1  the in-place step kernel builds the windows in the launch that steps, where that launch fuses nothing else: no LidarInFront
 *           observation, no action masks, no host write-through, and view_size <= 2 - a larger window costs the stepping wave more than the second
 *           launch does (the environment variable NGW_VIEW_FUSE=<view_size, at most 16> moves the limit for A/B runs).  Every other launch - those forms, the staged and the general
 *           kernel, resets, fused rollouts, larger windows - is followed by the stand-alone gather on the stream.  Same bytes either way.
 *   on = 2  the stand-alone gather behind every launch (the A/B form of on = 1).
 *   on = 0  off: the handle is back to gathering only when ngw_agent_view asks (view_size is ignored).
 * While it is on, the handle tracks whether the buffer describes the current state: ngw_agent_view(h, view_size) with the kept size launches nothing
 * when it does, and gathers again after a call that wrote the state some other way (ngw_set_state, a snapshot restore).  ngw_agent_view with ANOTHER
 * size gathers into a buffer of its own and leaves the kept windows alone; ngw_get_agent_view / ngw_agent_view_device_ptr answer for the last
 * ngw_agent_view call.  A one-env handle steps through per-launch kernels while it is on (the resident step loop has no view).  A captured graph is
 * dropped (it bakes the form in): build it after this call.
 * NGW_E_INVALID_ARG: a NULL handle; on outside 0..2; on != 0 with view_size outside 1..127 ("view_size must be in 1..127") or a buffer beyond the
 * 4 GiB index range. */
int ngw_agent_view_fuse(ngw_handle* h, int view_size, int on);

/* Action masks (invalid-action masking, the action_masks() convention of MaskablePPO): the mask of env i is a uint64 word, bit a = 1
 * exactly when step(a) taken from env i's CURRENT state (the state the next step acts on; after an autoreset, the new episode's first
 * state) would report result = 1 under the handle's spec, every novelty and wrapper predicate included; bits >= n_actions are 0.
 * The handle tracks whether its mask buffer describes the current state: reset, set_state, a rollout and steps taken with masks off
 * make it stale, and ngw_action_mask / ngw_get_action_mask recompute it (one kernel launch).
 * enable = 1: every following step (ngw_step*, the host steps, graphs built while it is on) also leaves the post-step masks, computed
 * inside the step kernel (with the fused lidar or the host write-through form: by the mask kernel right behind the step on the handle's
 * stream); ngw_step_device_many and a graph's replay compute them for their last step only.  0 = computed on demand only. */
int ngw_set_action_mask(ngw_handle* h, int enable);
/* makes the device buffer current (enqueued on the handle's stream; no launch when it is current already) */
int ngw_action_mask(ngw_handle* h);
/* [n_envs] words to host memory, made current first; waits for the stream.  A one-env handle whose resident step loop is running
 * answers from the outcomes the loop has speculated for every action of the current state: no launch, the loop keeps running. */
int ngw_get_action_mask(ngw_handle* h, uint64_t* out_host);
/* the device buffer: [n_envs] uint64 in HBM (call ngw_action_mask before reading it) */
int ngw_action_mask_device_ptr(ngw_handle* h, void** out);

/* Device-side snapshots: save, restore and fork env states by index, without leaving the device.
 * A snapshot is a device buffer of `capacity` slots that belongs to the handle that created it; a slot holds the full state of one env in
 * that handle's map size and item count - the seven arrays of ngw_get_state: map, agent_location, agent_facing_id, inventory, selected
 * item, step_count and the episode counter.  That is everything: `done` is a function of the inventory, and the reset stream is a
 * function of (seed, global env index, episode counter).  reward / done / info of the last step are NOT part of it: ngw_get_step_out
 * after a restore still reports the last step.  A slot that was never saved holds an all-zero row with agent_location (1, 1), a legal state.
 *   save     slot[slots[j]] := state[envs[j]]  for j < count.  The slots of one call must be distinct.
 *   restore  state[envs[j]] := slot[slots[j]]  for j < count.  Slots may repeat - that is the fork; the envs of one call must be
 *            distinct.  Envs not named keep every byte of their state.  flags: NGW_SNAP_KEEP_EPISODE leaves the destination env's
 *            episode counter as it is; without it the counter is restored with the rest.
 * Index lists are int32 arrays in DEVICE memory; NULL means 0 .. count-1.  An index outside [0, n_envs) / [0, capacity) makes that one
 * copy a no-op and raises the sticky NGW_F_BAD_INDEX (ngw_error_flags).  count above n_envs (restore) or capacity (save), a NULL handle or
 * snapshot, and a snapshot that is not an open snapshot of this handle return NGW_E_INVALID_ARG.
 * The future of a restored env: env e, when it next resets, draws from env e's OWN stream at its (restored or kept) episode counter.  Two
 * forks of one slot therefore share the rest of the current episode - same map, same actions, same outcomes - and differ from their next
 * reset on; restoring the same env from the same slot twice replays the same future, resets included.
 * Save and restore are enqueued on the handle's stream, like ngw_step_device, and do not wait.  A restore makes the action masks, the host
 * mirrors and the occupancy bit rows stale like ngw_set_state does, refreshes a fused lidar observation, and - unless the episode counters
 * were kept - is followed by a refill of the prepared next episodes, as ngw_reset is.  A captured graph stays valid.
 * ngw_snapshot_get copies `count` slots from `first` to host arrays shaped as for ngw_get_state (any may be NULL) and waits.
 * ngw_snapshot_destroy waits for the stream (queued copies may still read the buffer) and frees it; ngw_destroy frees what is still open. */
typedef struct ngw_snapshot ngw_snapshot;
#define NGW_SNAP_KEEP_EPISODE 1
int ngw_snapshot_create(ngw_handle* h, int64_t capacity, ngw_snapshot** out);
int ngw_snapshot_destroy(ngw_handle* h, ngw_snapshot* s);
int ngw_snapshot_save(ngw_handle* h, ngw_snapshot* s, const int32_t* envs_dev, const int32_t* slots_dev, int64_t count);
int ngw_snapshot_restore(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, const int32_t* envs_dev, int64_t count, int flags);
int ngw_snapshot_get(ngw_handle* h, ngw_snapshot* s, int64_t first, int64_t count, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv,
                     int32_t* selected, int32_t* step_count, uint32_t* episode);
/* Slot to slot, unchanged: slot dst_idx[j] of `dst` := slot src_idx[j] of `src` for j < count - the whole seven-array row, the episode counter
 * included (a search moves the children that turned out to be new from a scratch pool into an archive pool without committing them to an env).
 * Index lists are int32 arrays in DEVICE memory, NULL means 0 .. count-1; an index out of range skips that copy and raises NGW_F_BAD_INDEX.
 * Sources may repeat; the destinations of one call must be distinct.  src == dst is allowed when no destination of the call is also a source
 * of the same call (both lists NULL is then refused); a violated rule leaves those slots unspecified and never addresses out of bounds.
 * The same kernel as save and restore, one launch on the handle's stream; does not wait; nothing else changes.
 * NGW_E_INVALID_ARG: a NULL handle or snapshot; one that is not an open snapshot of this handle; count < 0 or above dst's capacity; src_idx == NULL
 * with count above src's capacity. */
int ngw_snapshot_copy(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, ngw_snapshot* dst, const int32_t* dst_idx_dev, int64_t count);

/* Snapshot expand: step saved states into new slots, commit nothing (the node expansion of a tree search: beam search, MCTS, archives of
 * states, breadth-first solvers - lookahead tables and plan evaluation return numbers and throw the stepped state away, this keeps it).
 * For j < count: the parent is row src_idx[j] - of snapshot `src`, or, with src == NULL, the handle's env src_idx[j] -, the child is the parent
 * stepped once with actions[j], and the child goes to slot dst_slots[j] of `dst`.  A NULL index list means 0 .. count-1, as in save and restore.
 * The child is the full seven-array row as the step leaves it BEFORE any reset: map, agent_location, agent_facing_id, inventory and selected
 * carry the step's effects (the one cell write, the 3 x 3 pick-up, Crate contents, a craft's inputs and output, a move, turn or jump),
 * step_count is what the step leaves (+1, or +2 where FenceRestriction's epilogue counts twice), episode is the parent's.  No reset runs: the
 * child of a step that ends the episode (goal, FireWall death, the horizon under autoreset) is the state the episode ended in - what terminal
 * capture would store.  The rules are exactly those of ngw_step_device under the handle's spec, every novelty and wrapper predicate, and its
 * autoreset setting and horizon.
 * reward[j], done[j], info[j] (device memory, [count], any may be NULL) are what ngw_get_step_out would report for that step (the NGW_INFO_*
 * packing); when the parent is env i's current state they equal entry (i, actions[j]) of the lookahead table.  The sticky done of a parent
 * that already holds the goal item, with autoreset off, is reported as the step reports it; expanding an ended node is the caller's business.
 * An action id outside [0, n_actions) behaves as in ngw_plan_eval: the child is a copy of the parent, reward, done and info are 0, and the
 * sticky NGW_F_INVALID_ACTION is raised.
 * A parent or destination index out of range skips that pair - nothing is stored, its reports are left untouched - and raises the sticky
 * NGW_F_BAD_INDEX; nothing is ever addressed with it.  Parents may repeat (the fan-out); the destination slots of one call must be distinct.
 * src == dst is allowed (a node pool in one buffer): then no destination slot of the call may also be a parent of the same call.  Device
 * index lists are used in place, unchecked beyond range: a violated distinctness rule leaves those slots' contents unspecified and never
 * causes an out-of-bounds access.
 * Nothing is committed (the lookahead's list holds in full): every byte of every env's state, the last step's reward / done / info, the
 * prepared next episodes, the mask buffer and the lookahead table and whether each is current, the lidar rows, the bit rows, the host mirrors,
 * the rollout output rows and accumulators, the terminal-capture side set, and every slot of every snapshot that the call does not name as a
 * destination are what they were.  Because no reset runs, the call is allowed while terminal capture is on.
 * One kernel launch, enqueued on the handle's stream; does not wait.  A captured graph stays valid.  count == 0 is a no-op.
 * NGW_E_INVALID_ARG: a NULL handle, dst or actions; a src or dst that is not an open snapshot of this handle; count < 0 or above dst's
 * capacity; src_idx == NULL with count above the source's row count (src's capacity, or n_envs); maps that do not fit LDS (the kernel keeps
 * a wavefront's 64 rows there, the fused rollouts' limit). */
int ngw_snapshot_expand(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, ngw_snapshot* dst,
                        const int32_t* dst_slots_dev, int64_t count, int32_t* reward_dev, uint8_t* done_dev, uint32_t* info_dev);

/* Snapshot rollout: roll action sequences out from saved states; optionally keep the end state.  It closes the gap between ngw_plan_eval
 * (T-step sequences, but only from the envs' current states, and the stepped state is thrown away) and ngw_snapshot_expand (any saved slot, the
 * stepped state kept, but exactly one step): the leaf simulation of a tree search that keeps its nodes in a snapshot pool, and the macro-action
 * of T steps applied to a node.
 * For j < count: the parent is row src_idx[j] of snapshot `src`, or, with src == NULL, the handle's env src_idx[j] (its current state).  A NULL
 * index list means 0 .. count-1, as in ngw_snapshot_expand.  The action of pair j at step t is actions_dev[t * pair_stride + j], int32 in device
 * memory, pair_stride >= count (step-major: 64 lanes read consecutive addresses).
 * The pair is stepped from its parent on a private copy by exactly ngw_plan_eval's rules: the handle's spec, every novelty and wrapper
 * predicate, and its autoreset setting and horizon apply; it STOPS at the first step whose `done` would be 1 - the goal (including the sticky
 * done of a parent that already holds the goal item, with autoreset off), a FireWall death, or the horizon under autoreset -, that ending step
 * counts, and no reset ever runs.
 * ret[j] (int32: the sum of the executed steps' rewards), length[j] (int32: steps executed, 1 .. n_steps), ended[j] (uint8: the pair stopped at
 * an episode end) and info[j] (uint32: the NGW_INFO_* word of the last executed step) - device memory, [count] - are as ngw_plan_eval defines
 * them.  Any of the four pointers may be NULL.
 * With dst != NULL, slot dst_slots[j] of `dst` (dst_slots == NULL: slots 0 .. count-1) receives the full seven-array row as the LAST EXECUTED
 * step leaves it, by ngw_snapshot_expand's definition of a child: map, agent_location, agent_facing_id, inventory and selected carry the
 * steps' effects, step_count is as the steps left it, episode is the parent's, and for a stopped pair the row is the state the episode ended
 * in.  dst == NULL keeps nothing - a pure evaluation -, and dst_slots must then be NULL as well.
 * An action id outside [0, n_actions) follows the plan convention: the step leaves the private state untouched, adds reward 0, counts in
 * `length`, has info word 0, and raises the sticky NGW_F_INVALID_ACTION only while the pair is still running.
 * A parent or destination index out of range follows ngw_snapshot_expand's convention: the pair is skipped - nothing is stored for it, its
 * reports are left untouched -, the sticky NGW_F_BAD_INDEX is raised, and nothing is ever addressed with the bad index.
 * Parents may repeat; the destination slots of one call must be distinct.  src == dst is allowed when no destination slot of the call is also a
 * parent of the same call.  Device lists are used in place, unchecked beyond range: a violated rule leaves those slots' contents unspecified
 * and never causes an out-of-bounds access.
 * Nothing is committed - ngw_snapshot_expand's list holds word for word: every byte of every env's state, the last step's reward / done / info,
 * the prepared next episodes (no step counts against the refill cadence), the mask buffer and the lookahead table and whether each is current,
 * the lidar rows, the bit rows, the host mirrors, the rollout output rows and accumulators, the terminal-capture side set, and every slot of
 * every snapshot that the call does not name as a destination are what they were.  Because no reset runs, the call is allowed while terminal
 * capture is on.
 * One kernel launch, enqueued on the handle's stream; does not wait.  A captured graph stays valid.  count == 0 is a no-op.
 * Two identities hold:
 *   - n_steps == 1 with dst given: the children and the reports equal ngw_snapshot_expand's for the same pairs, ret = its reward and
 *     ended = its done (length is 1);
 *   - src == NULL, dst == NULL and src_idx = the envs 0 .. n_envs-1: the reports equal the column ngw_plan_eval computes for the same plan.
 * NGW_E_INVALID_ARG: a NULL handle or NULL actions; n_steps < 1; count < 0; pair_stride < count; dst == NULL with all four report pointers NULL
 * (nothing to do); dst == NULL with dst_slots != NULL; a src or dst that is not an open snapshot of this handle; count above dst's capacity;
 * src_idx == NULL with count above the source's row count (src's capacity, or n_envs); maps that do not fit LDS (the kernel keeps a
 * wavefront's 64 rows there, the fused rollouts' limit). */
int ngw_snapshot_rollout(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                         ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev,
                         uint32_t* info_dev);

/* Slot observations: the observation and the valid-action mask of SAVED states, gathered by slot index - the read-only side of a node pool
 * (policy- or value-guided tree search, beam search with a learned scorer, cell descriptors of an archive: every node that is evaluated needs
 * its observation and its mask, and restoring it into an env to look at it would commit state).
 * `s` is an open snapshot of `h`; slots_dev is an int32 list in DEVICE memory, NULL means 0 .. count-1.  Slots may repeat, and count is not bound
 * by the capacity unless slots_dev == NULL.  Output row j describes slot slots[j].
 *   ngw_snapshot_lidar        row j of rows_dev is the LidarInFront observation of slot slots[j] under the handle's current configuration
 *                             (ngw_lidar_configure) and current row format (ngw_lidar_set_output: 32 / 16 / 8 = packed, ngw_lidar_row_layout), bit-identical to
 *                             what ngw_lidar + ngw_lidar_device_ptr give for an env that holds that state.  rows_dev has room for `count` ROUNDED UP TO A
 *                             MULTIPLE OF 64 rows; rows past count are unspecified.  It always runs the march over maps staged in LDS (the stand-alone
 *                             launch's form, whichever form the env's fused path uses: slots have no occupancy bit rows and get none).
 *                             NGW_E_INVALID_ARG before ngw_lidar_configure, and where ngw_lidar is refused (maps that do not fit LDS).
 *   ngw_snapshot_agent_view   view_dev is int8 [count][W][W], W = 2 * view_size + 1, 0 outside the map: the AgentMap window of each slot; view_size has
 *                             ngw_agent_view's limits (1 .. 127, and the byte count within the 4 GiB index range); the buffer is rounded up to a whole
 *                             dword.  facing_dev [count] and inv_dev [count][n_items] are the other two entries of that wrapper's observation, gathered in
 *                             the same launch.  Any of the three pointers may be NULL, but not all of them.
 *   ngw_snapshot_action_mask  masks_dev[j] is the uint64 mask of slot slots[j]: bit a is set exactly when step(a) from that state would report result = 1
 *                             under the handle's spec, every novelty and wrapper predicate included (the predicate of ngw_action_mask); bits >=
 *                             n_actions are 0.
 * A slot index outside [0, capacity) is never used as an address: its output row is all zeros (mask 0, facing 0), and the sticky NGW_F_BAD_INDEX is
 * raised.  count == 0 is a no-op.  Each call is ONE kernel launch, enqueued on the handle's stream; it does not wait.
 * Nothing is committed - ngw_snapshot_expand's list holds word for word: every byte of every env's state, the last step's reward / done / info,
 * the prepared next episodes, the mask buffer and the lookahead table and whether each is current, the lidar rows, the bit rows, the host mirrors,
 * the rollout output rows and accumulators, the terminal-capture side set, and every slot of every snapshot are what they were.  In addition the
 * env's own lidar buffer (ngw_lidar_device_ptr), agent-view buffer and mask buffer are not touched, and whether each is current does not change.
 * A captured graph stays valid.  The calls are allowed with the fused lidar, the bit-row form, masks-in-step and terminal capture on.
 * NGW_E_INVALID_ARG: a NULL handle, snapshot or output (agent view: all three outputs NULL); a snapshot that is not an open snapshot of this
 * handle; count < 0; slots_dev == NULL with count above the capacity. */
int ngw_snapshot_lidar(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, void* rows_dev);
int ngw_snapshot_agent_view(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, int view_size, int8_t* view_dev, int32_t* facing_dev,
                            int32_t* inv_dev);
int ngw_snapshot_action_mask(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, uint64_t* masks_dev);

/* State keys: a 64-bit key of a saved slot or of an env's current state, computed on the device - "are these two nodes the same state?" for
 * transposition tables, duplicate removal, archives keyed by a cell descriptor, visit counts.  The key is a public contract, so a caller can
 * compute the same key on the host for a state read with ngw_get_state / ngw_snapshot_get.  All arithmetic is uint64, wrapping:
 *     mix64(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     term(tag, index, value) = mix64((uint64)tag << 56 | (uint64)index << 32 | (uint32)value)
 * and key(row, fields) is the XOR of the terms of the fields selected in `fields`:
 *   NGW_KEY_MAP         for each group g = 0 .. ceil(S*S / 4) - 1: w = the little-endian uint32 of cells 4g .. 4g+3 of the row-major int8 map (cells
 *                       past S*S count as 0; cell 0 is the row's first cell, wherever the row lies in memory); if w != 0: term(1, g, w)
 *   NGW_KEY_POSE        term(2, 0, r | c << 8 | facing << 16)
 *   NGW_KEY_INV         for each item k with inv[k] != 0: term(3, k, inv[k])
 *   NGW_KEY_SELECTED    term(4, 0, selected)      (also when selected is 0)
 *   NGW_KEY_STEP_COUNT  term(5, 0, step_count)
 *   NGW_KEY_EPISODE     term(6, 0, episode)
 * Every term is independent, so a key can be updated incrementally: changing one cell XORs its group's old term out and the new one in.
 * NGW_KEY_STATE (the default of the Python layer) is the Markov state with autoreset off; add NGW_KEY_STEP_COUNT where a horizon applies;
 * NGW_KEY_POSE | NGW_KEY_INV is a typical Go-Explore cell.  A never-saved slot has the key 0x43fc77d84676ced7 under NGW_KEY_STATE. */
#define NGW_KEY_MAP 1u
#define NGW_KEY_POSE 2u
#define NGW_KEY_INV 4u
#define NGW_KEY_SELECTED 8u
#define NGW_KEY_STEP_COUNT 16u
#define NGW_KEY_EPISODE 32u
#define NGW_KEY_STATE 15u       /* map | pose | inventory | selected item */
#define NGW_KEY_ALL 63u
/* keys_dev[j] = key(row idx[j], fields), `count` of them.  `s` is an open snapshot of `h` (rows = its slots); with s == NULL the rows are the
 * handle's envs' CURRENT states (n_envs rows), as a NULL `src` of ngw_snapshot_expand (a one-env handle's resident step loop is ended first: HBM
 * holds the state only once it has).  idx_dev is an int32 list in DEVICE memory, NULL means 0 .. count-1 (count may then not exceed the row
 * count); indices may repeat, and count is otherwise not bound by the row count.  An index outside [0, rows) is never used as an address: its key
 * is 0 and the sticky NGW_F_BAD_INDEX is raised.  Exactly keys_dev[0 .. count) is written.  count == 0 is a no-op.
 * ONE kernel launch (ngw_keys.inc), enqueued on the handle's stream; it does not wait.  It stages nothing in LDS and works at every map size.
 * Nothing is committed - the slot observations' list holds word for word: every byte of every env's state, the last step's outputs, the
 * prepared next episodes, the mask, lookahead, lidar and view buffers and whether each is current, the bit rows, the host mirrors and every slot
 * of every snapshot are what they were.  A captured graph stays valid.
 * NGW_E_INVALID_ARG: a NULL handle or output; a snapshot that is not an open snapshot of this handle; count < 0; fields == 0 or a bit above
 * NGW_KEY_ALL; idx_dev == NULL with count above the row count. */
int ngw_state_keys(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, uint32_t fields, uint64_t* keys_dev);

/* Successor keys: the key of every action's child, with no child stored - "which of this node's children are new?" before any of them is written.
 * With A = the spec's n_actions, for j < count and a < A:
 *     keys_dev[j * A + a] = exactly the key ngw_state_keys(..., fields) would return for the child ngw_snapshot_expand would write for parent idx[j]
 *                           and action a (the state the step leaves before any reset; the episode counter is the parent's; NGW_KEY_STEP_COUNT sees
 *                           the stepped count),
 *     reward_dev / done_dev / info_dev [j * A + a] (each NULL or [count][A]) = exactly what that expand would report, under the handle's autoreset
 *                           setting and horizon.
 * Position j * A + a is the pair numbering of an expand of every action, so the flattened keys go straight into ngw_key_table_insert and a fresh
 * position maps back to (parent, action) by division.  `s`, idx_dev, count and the index rules are ngw_state_keys': s == NULL means the envs'
 * current states; idx_dev is an int32 list in DEVICE memory, NULL means 0 .. count-1 (count may then not exceed the row count); parents may repeat
 * and count is otherwise not bound by the row count; an index outside [0, rows) is never used as an address: its A keys are 0 (which the key table
 * never stores), its reports are 0, and the sticky NGW_F_BAD_INDEX is raised.  Exactly [0, count * A) of each given array is written.
 * ONE kernel launch (ngw_successors.inc), enqueued on the handle's stream; it does not wait.  It keeps two sets of a wavefront's 64 rows in LDS
 * (the stepped rows and the parents they are compared with): 2 * 64 * (MS + 4 * KP) bytes, MS = the map's LDS stride, KP = n_items | 1.  That fits
 * the 160 KiB of a CU for every map_size up to 34 in every configuration; a handle with larger maps is refused (NGW_E_INVALID_ARG), and
 * ngw_snapshot_expand followed by ngw_state_keys remains.
 * Nothing is committed, as for ngw_state_keys: no env, slot, mask, lookahead table, mirror or prepared episode changes, and a captured graph
 * stays valid.
 * NGW_E_INVALID_ARG: a NULL handle or keys_dev; a snapshot that is not an open snapshot of this handle; fields == 0 or a bit above NGW_KEY_ALL;
 * count < 0; idx_dev == NULL with count above the row count; count * A beyond the index range of a launch (2^31 - 1 wavefronts of keys); maps
 * the call cannot hold. */
int ngw_successor_keys(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, uint32_t fields, uint64_t* keys_dev, int32_t* reward_dev,
                       uint8_t* done_dev, uint32_t* info_dev);

/* Walk distances and go-to plans: "how many primitive steps until the agent can face item k, and which ones?" - the macro-action "go to the nearest
 * X and face it" for ngw_snapshot_rollout, an admissible heuristic for a best-first search over a node pool, a shaping potential, a feature vector.
 * The quantity is a public integer contract, defined on the saved state alone - the map bytes and the pose - under the BASE movement rules:
 *   facing:  NORTH 0, SOUTH 1, WEST 2, EAST 3;    dr = {-1, 1, 0, 0}, dc = {0, 0, -1, 1};    left = {2, 3, 1, 0}, right = {3, 2, 0, 1}
 *   A pose is (r, c, f).  Three moves, each of cost 1:
 *     Forward  (r, c, f) -> (r + dr[f], c + dc[f], f)   if and only if that cell lies inside the map and holds id 0
 *     Left     (r, c, f) -> (r, c, left[f])             Right    (r, c, f) -> (r, c, right[f])
 *   D(p) = the breadth-first distance of pose p from the agent's pose (agent_location, agent_facing_id) over these moves; D(agent's pose) = 0
 *   whatever the agent's own cell holds.  The map is static: no pickup, no novelty predicate enters the rule, so under a Jump action or a
 *   FireWall / FenceRestriction / Crate predicate this is a geometric quantity, not a promise about what step() does.
 *   front(p) = the id of the cell (r + dr[f], c + dc[f]); a pose whose front cell lies outside the map has none.
 *   dist[k], for every item id k in [0, n_items) - air 0 and wall are ordinary columns - = min D(p) over the reachable poses with front(p) == k:
 *     0 when the agent already faces a k cell, -1 when no reachable pose faces one.
 *   goal(k) = the reachable pose with front(p) == k that minimises the tuple (D, r, c, f) lexicographically.
 *   path(k): walk back from q = goal(k) to the agent's pose.  At a pose q = (r, c, f) with D(q) = d > 0 take the FIRST of these predecessors p:
 *     1. the Forward predecessor p = (r - dr[f], c - dc[f], f), if p lies inside the map, is reachable with D(p) = d - 1, and Forward leads from p to
 *        q (q's cell holds id 0 - every pose with d > 0 outside the agent's own cell does);
 *     2. the pose that reaches q by Left, p = (r, c, right[f]), if D(p) = d - 1;
 *     3. the pose that reaches q by Right, p = (r, c, left[f]) (then D(p) = d - 1: q has a predecessor in layer d - 1).
 *     and continue from p.  The plan is the moves taken, reversed: the first move leaves the agent's pose, the last one arrives at goal(k).
 *   The ids a plan is written in are the LOWEST action id whose act_kind is NGW_ACT_FORWARD, NGW_ACT_LEFT and NGW_ACT_RIGHT respectively, so a
 *   remapped action table is honoured.
 * For j < count, with K = n_items and T = n_steps:
 *     dist_dev[j * K + k]        (int32, NULL or [count][K])  = dist[k] of row idx[j]
 *     length_dev[j]              (int32, NULL or [count])     = dist[items_dev[j]]: the TRUE length, also beyond T
 *     plans_dev[t * count + j]   (int32, NULL or [T][count])  = move t of path(items_dev[j]) for t < min(length, T), -1 elsewhere - the step-major layout
 *                                and the padding of ngw_snapshot_playout's actions_dev, which ngw_snapshot_rollout reads as actions_dev with
 *                                pair_stride = count.  A path longer than T gives its first T moves; an unreachable item a column of -1.
 * What gives this its value: on a configuration whose Forward is the base rule, ngw_snapshot_rollout_path of these plans with limits = length clamped
 * to [0, T] leaves child j facing a cell of id items_dev[j] after exactly length[j] steps, each with result == true.
 * `s`, idx_dev, count and the index rules are ngw_state_keys': s == NULL means the envs' current states; idx_dev is an int32 list in DEVICE memory,
 * NULL means 0 .. count-1 (count may then not exceed the row count); rows may repeat and count is otherwise not bound by the row count.  items_dev is
 * an int32 list in DEVICE memory, one item id per row; NULL asks for the distances alone (plans_dev and length_dev must then be NULL, n_steps is not
 * read) and skips the walk back.  An index outside [0, rows), or an item outside [0, n_items), is never used as an address: every output of that row
 * is -1 (its K distances, its length, its column of plans) and the sticky NGW_F_BAD_INDEX is raised.  Exactly the ranges above are written.
 * ONE kernel launch (ngw_walk.inc), enqueued on the handle's stream; it does not wait.  One wavefront serves one row and stages that one map, so it
 * works at every map size up to 64 x 64 within the default 64 KiB of LDS.  count == 0 is a no-op.
 * Nothing is committed, as for ngw_state_keys: no env, slot, mask, lookahead table, mirror or prepared episode changes, and a captured graph
 * stays valid.
 * NGW_E_INVALID_ARG: a NULL handle; no output pointer at all; a snapshot that is not an open snapshot of this handle; count < 0 or beyond 2^31 - 1;
 * idx_dev == NULL with count above the row count; plans_dev or length_dev without items_dev; items_dev with n_steps < 1; plans_dev on a spec that lacks
 * a Forward, a Left or a Right action (the distances are still served). */
int ngw_snapshot_walk(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, const int32_t* items_dev, int32_t n_steps, int32_t* dist_dev,
                      int32_t* plans_dev, int32_t* length_dev);

/* Playouts: "from this node, play n_steps steps of a random policy and report what happened" - the default-policy simulation of MCTS, flat
 * Monte-Carlo and Go-Explore.  The policy is uniform over the actions that WOULD SUCCEED from the state the pair is in at that step, which
 * only the device knows inside a rollout; the actions are therefore drawn in the kernel.  The choice is a public contract, like the state
 * key, so a host can reproduce any playout from (seed, pair number, step) and the state.  For pair j of a call - global pair number
 * p = first_pair + j, a uint64 - at step t (0-based):
 *     m  = the valid-action mask word of the pair's state before step t: bit a is set exactly when step(a) would report result = 1 (the
 *          predicate of ngw_action_mask / ngw_snapshot_action_mask);  if m == 0 (no action would succeed): m = all n_actions bits
 *     n  = popcount(m)
 *     w  = word (t & 3) of Philox4x32-10 with counter (t >> 2, 0, lo32(p), hi32(p)) and key (lo32(seed), hi32(seed) ^ NGW_PLAYOUT_TAG) - the
 *          generator and word order of ngw_rollout under another tag: a playout and a fused rollout of one seed are unrelated
 *     k  = ((uint64)w * n) >> 32;  the action is the id of the (k + 1)-th set bit of m, counted from bit 0.
 * The draw depends on (seed, p, t) and the state only: not on the slot, the env index, the rank, how the pairs fall into wavefronts, or how
 * many steps earlier calls ran.
 * Everything else follows ngw_snapshot_rollout: src / src_idx_dev / dst / dst_slots_dev / count mean what they mean there (src == NULL: the
 * envs' current states; dst == NULL: nothing is kept, and dst_slots_dev must then be NULL); the pair steps a private copy of the parent row, it
 * stops at the first step whose `done` would be 1 (goal, FireWall death, the horizon under autoreset), that step counts, no reset ever runs,
 * and an ended pair draws nothing more.  ret / length / ended / info take element j as ngw_snapshot_rollout defines them; first_action_dev[j]
 * (int32) is the action of step 0 - what a flat Monte-Carlo search groups the returns by -; actions_dev (int32) takes the action of pair j at
 * step t at [t * actions_stride + j], the layout ngw_snapshot_rollout reads, so a recorded playout can be replayed; a step the pair did not
 * execute holds -1.  Every output pointer may be NULL.
 * A parent or destination index out of range skips the pair: nothing is ever addressed with the bad index, its four reports are stored as 0,
 * its first action and its column of actions_dev as -1, no slot is written for it, and the sticky NGW_F_BAD_INDEX is raised.
 * Nothing is committed - ngw_snapshot_rollout's list holds word for word.  One kernel launch (ngw_playout.inc), enqueued on the handle's
 * stream; does not wait.  A captured graph stays valid.  count == 0 is a no-op.  A one-env handle's resident step loop is ended first.
 * NGW_E_INVALID_ARG: a NULL handle; n_steps < 1; count < 0; actions_dev given with actions_stride < count; dst == NULL with dst_slots_dev !=
 * NULL; a src or dst that is not an open snapshot of this handle; count above dst's capacity; src_idx_dev == NULL with count above the source's
 * row count; maps that do not fit LDS (ngw_snapshot_rollout's limit). */
#define NGW_PLAYOUT_TAG 0x504C4159u
int ngw_snapshot_playout(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                         ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                         int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride);

/* Weighted choice among valid actions: "for each state, pick an action with probability proportional to my weight, among the actions the state
 * accepts" - invalid-action masking as a policy-gradient loop, a policy-guided tree search and a biased ("heavy") playout need it, in one
 * launch.  The choice is a public contract, like the playout rule above, in integers and IEEE binary32, so a host reproduces it bit for bit.
 * For pair j of a call - global pair number p = first_pair + j, a uint64 - at step number t, with the caller's float32 weights x[a]:
 *   1. m  = the valid-action mask word of the pair's state (the predicate of ngw_action_mask, every novelty and wrapper predicate included);
 *           if m == 0: m = all n_actions bits.  This is the playout rule's m.
 *   2. w  = word (t & 3) of Philox4x32-10 with counter (t >> 2, 0, lo32(p), hi32(p)) and key (lo32(seed), hi32(seed) ^ NGW_SAMPLE_TAG).
 *   3. the cleaned weight v[a], a < n_actions: x[a] if bit a of m is set and 2^-64 <= x[a] <= 2^64, else +0.  A weight that is negative, NaN or
 *      above 2^64 (infinity included) raises the sticky NGW_F_BAD_WEIGHT, whether or not action a is valid; a weight in [0, 2^-64) is silently 0
 *      (an underflowed softmax is legitimate; -0.0 compares equal to 0 and is such a weight).
 *   4. c[-1] = 0, c[a] = c[a-1] + v[a] in binary32, round-to-nearest-even, in action order, every add a plain add (never fused with a
 *      multiply);  mass = c[n_actions - 1].
 *   5. mass > 0:  u = float(w >> 8) * 2^-24 (exact, in [0, 1));  thr = u * mass (one binary32 multiply);  the action is the smallest a with
 *      v[a] > 0 and c[a] > thr.  The bounds of rule 3 keep every intermediate normal and finite for up to 48 actions, so no flush-to-zero or
 *      overflow question arises; thr < mass always holds - should no a qualify, the action is the last a with v[a] > 0.
 *   6. mass == 0: the playout rule on this w:  k = ((uint64)w * popcount(m)) >> 32, the (k + 1)-th set bit of m; mass is reported as 0.
 * The draw depends on (seed, p, t), the state and the weights only: not on the slot, the env index, the rank or the wavefront.  mass is returned
 * so that the caller forms log pi(a) = log x[a] - log mass itself: the kernel divides nothing and calls no transcendental function.
 *
 * ngw_sample_actions: src == NULL: the envs' current states, else a snapshot's slots; idx_dev: int32 row indices in device memory (NULL =
 * 0 .. count-1; indices may repeat, count is not bound by the row count with a list).  weights_dev: float32 in device memory, action-major:
 * x[a] of pair j at [a * weight_stride + j], weight_stride >= count.  actions_dev[j] (int32) = the action, mass_dev[j] (float32, may be NULL) =
 * mass, masks_dev[j] (uint64, may be NULL) = m as rule 1 defines it - the word a learner stores to recompute masked log-probabilities.
 * A row index out of range is never used as an address: that pair gets action -1, mass 0 and mask 0, and the sticky NGW_F_BAD_INDEX is raised
 * (its weights are still checked for NGW_F_BAD_WEIGHT).  One kernel launch (ngw_sample.inc) on the handle's stream; does not wait.  A
 * captured graph stays valid.  count == 0 is a no-op.  Map cells are read in place: every map size the handle supports.  Nothing is committed:
 * no env state, no step output, no mask buffer or its currency, no lookahead table, no lidar row, no prepared episode and no slot changes -
 * ngw_snapshot_action_mask's list word for word.  A one-env handle's resident step loop is ended first.
 * NGW_E_INVALID_ARG: a NULL handle, weights_dev or actions_dev; count < 0; weight_stride < count; a src that is not an open snapshot of this
 * handle; idx_dev == NULL with count above the source's row count. */
#define NGW_SAMPLE_TAG 0x53414D50u
int ngw_sample_actions(ngw_handle* h, ngw_snapshot* src, const int32_t* idx_dev, int64_t count, const float* weights_dev, int64_t weight_stride,
                       uint64_t seed, uint64_t first_pair, uint32_t t, int32_t* actions_dev, float* mass_dev, uint64_t* masks_dev);

/* ngw_snapshot_playout with a weighted policy: weights_dev = n_actions float32 in device memory, one per action, the same for every pair and
 * step.  Every step's choice is rules 3 - 6 above applied to the playout's own m and its own w (NGW_PLAYOUT_TAG and the playout's counter, both
 * unchanged): proportional to the weights among the valid actions, the uniform rule where their mass is 0.  A bad weight raises
 * NGW_F_BAD_WEIGHT.  Everything else - arguments, reports, errors, the map-size limit - is ngw_snapshot_playout's; weights_dev == NULL is
 * that call. */
int ngw_snapshot_playout_weighted(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed,
                                  uint64_t first_pair, const float* weights_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                                  int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev,
                                  int64_t actions_stride);

/* Path keys and per-pair step limits: ngw_snapshot_rollout / ngw_snapshot_playout(_weighted) that also report the key of EVERY state a pair
 * passes through, not only where it stops - what a Go-Explore archive (every new cell along an exploration run), a per-step visit count and
 * loop detection inside a playout need, without stepping one step at a time.
 * Path keys (keys_dev != NULL).  For pair j and step t in 0 .. n_steps-1:
 *   keys_dev[t * keys_stride + j] (uint64, device memory, keys_stride >= count) = the key under `fields` (ngw_state_keys) of the state pair j is
 *   in after it has executed step t: bit for bit what ngw_state_keys returns for the slot the same call would write into dst for pair j if the
 *   pair stopped after step t.  The state after an ending step is the state the episode ended in, as ngw_snapshot_expand / ngw_snapshot_rollout
 *   define a child: NGW_KEY_EPISODE uses the parent's episode counter, NGW_KEY_STEP_COUNT the step count after step t (FenceRestriction's
 *   second count included); cells past S*S in the last map group count as 0, as everywhere.
 *   The key is 0 for every step the pair did not execute: after its episode ended, beyond its limit, or for a pair skipped with
 *   NGW_F_BAD_INDEX.  0 is the value the key table never stores, so the flattened [n_steps * keys_stride] array can be offered to
 *   ngw_key_table_insert / _lookup as it is, and position t * count + j makes "fresh" mean "the earliest step that reached it".
 *   Exactly [t * keys_stride, t * keys_stride + count) of every step row t < n_steps is written.
 * Limits (limits_dev != NULL: int32 [count], device memory).  Pair j executes at most min(n_steps, max(limits_dev[j], 0)) steps; values
 *   outside [0, n_steps] are clamped, no flag is raised.  A pair cut by its limit is NOT `ended`; its info is the word of its last executed
 *   step.  A limit of 0 gives length = ret = info = 0 and, with a destination, an unchanged copy of the parent.  In a playout the draws depend
 *   on (seed, p, t) and the state only, so a limited playout is the prefix of the unlimited one, and recorded actions beyond the limit are -1.
 *   With limits[j] = t + 1, a replay of the recorded actions through ngw_snapshot_rollout_path leaves in dst exactly the state whose key is
 *   keys[t * keys_stride + j].
 * keys_dev may be NULL (limits only; fields is then ignored) and limits_dev may be NULL; with both NULL the calls compute what the plain calls
 * compute.  A rollout with keys_dev needs neither a destination nor a report.  weights_dev == NULL is the uniform rule.  Everything else -
 * arguments, reports, index rules, ordering, the stream, what is (not) committed: nothing - is the plain calls'.  One kernel launch
 * (ngw_slot_rollout.inc / ngw_playout.inc in their PATH form, ngw_path.inc): the running key is updated for the dwords a step changes, no
 * row leaves LDS.  Map sizes: the calls keep one set of a wavefront's 64 rows in LDS, as the plain calls do, and 64 * (K | 1) dwords of
 * inventory shadows behind it; they serve every configuration whose two together fit 160 KiB - every configuration up to 32 x 32 and well
 * beyond; a handle within those last 256 * (K | 1) bytes of the plain calls' own limit is refused here while the plain calls still run.
 * NGW_E_INVALID_ARG: what the plain calls refuse; keys_dev with fields == 0 or a bit outside NGW_KEY_ALL; keys_dev with keys_stride < count;
 * rows and shadows that do not fit LDS. */
int ngw_snapshot_rollout_path(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                              const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev,
                              uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride);
int ngw_snapshot_playout_path(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                              const float* weights_dev /* NULL: the uniform rule */, const int32_t* limits_dev, ngw_snapshot* dst,
                              const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                              int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride, uint32_t fields, uint64_t* keys_dev,
                              int64_t keys_stride);

/* Trajectories: ngw_snapshot_rollout_path / ngw_snapshot_playout_path that also record every step of every pair - the reward, the mask word the
 * choice was made under, and the LidarInFront observation before and after it - so that the runs of a search are a dataset (behaviour cloning,
 * offline RL, value targets, a world model) without replaying them one step at a time through saved slots.  All arrays are device memory; each is
 * recorded only where its pointer is not NULL.  A pair EXECUTES step t while it is not skipped (NGW_F_BAD_INDEX), t is below its limit and no
 * earlier step ended its episode.
 * Rewards (rewards_dev != NULL; int32).  rewards_dev[t * rewards_stride + j], rewards_stride >= count: the reward of step t of pair j, 0 for a
 *   step it did not execute; the column of pair j sums to ret[j].  Exactly [t * rewards_stride, t * rewards_stride + count) of every step row
 *   t < n_steps is written.
 * Masks (masks_dev != NULL; uint64; playouts).  masks_dev[t * masks_stride + j], masks_stride >= count: the valid-action word m of the state pair j
 *   was in before step t, AFTER rule 1's replacement (all n_actions bits where no action would succeed) - the word the choice rule of
 *   ngw_snapshot_playout / rules 3 - 6 of ngw_sample_actions were applied to, so the rule on (m, seed, first_pair + j, t) reproduces the recorded
 *   action.  0 for a step the pair did not execute.  Written like the rewards.
 * Observations (obs_dev != NULL).  Rows of the handle's current lidar format (ngw_lidar_row_layout: row_bytes each; packed, int16 or int32), the
 *   rows ngw_snapshot_lidar returns for a slot holding that state.  Row numbering: the buffer is n_steps + 1 ROW BLOCKS of obs_stride rows;
 *   row j of block 0 is the observation of the parent of pair j, row j of block t + 1 the observation of the state step t leaves - before any
 *   reset, as every slot call defines a child: the last non-zero row of an ended pair shows the state its episode ended in.  A row is all zeros
 *   for a step the pair did not execute, and in every block - block 0 included - for a skipped pair.  So (row t, action t, reward t, row t + 1)
 *   is a transition for t < length[j].  One wavefront serves 64 consecutive pairs and stores its 64 rows of a block as ONE tile: obs_stride must
 *   be a multiple of 64 and at least count rounded up to 64, obs_dev 16-byte aligned, and rows count .. of every block (up to the next multiple
 *   of 64) are written with zeros; rows beyond that are not touched.  The buffer is (n_steps + 1) * obs_stride * row_bytes bytes: 65 536 pairs
 *   of 64 steps with 80-byte rows are 340 MB.  ngw_lidar_configure must have been called; the env's own lidar rows are not touched.
 * With the three pointers NULL the calls compute what the path calls compute.  A rollout with rewards_dev or obs_dev needs neither a destination
 * nor a report.  Everything else - limits, keys, arguments, reports, index rules, ordering, the stream, what is committed: nothing - is the path
 * calls'.  One kernel launch (ngw_slot_rollout.inc / ngw_playout.inc in their TRAJ form, ngw_traj.inc); no row leaves LDS.
 * Map sizes.  Without obs_dev: the path calls' layout and limit.  With obs_dev the wavefront's 64 rows lie in the layout of the stand-alone lidar
 *   launch (ngw_lidar / ngw_snapshot_lidar: the item tables, an 8 KiB ray table unless the rays are world-frame, the tile of 64 rows, the maps
 *   between two guards of max_range * (S + 1) bytes, the inventories), with the 64 * (K | 1) dwords of inventory shadows behind it where keys_dev
 *   is set too; a handle whose layout exceeds 160 KiB is refused (the message starts with "map_size" and names the bytes) while the call without
 *   obs_dev still runs.  Every configuration up to 32 x 32 fits, in every row format.
 * NGW_E_INVALID_ARG: what the path calls refuse; rewards_stride / masks_stride < count; obs_dev before ngw_lidar_configure, misaligned, or with
 * an obs_stride that is no multiple of 64 or below count rounded up to 64; a layout that does not fit LDS. */
int ngw_snapshot_rollout_traj(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                              const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev,
                              uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev,
                              int64_t rewards_stride, void* obs_dev, int64_t obs_stride);
int ngw_snapshot_playout_traj(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                              const float* weights_dev /* NULL: the uniform rule */, const int32_t* limits_dev, ngw_snapshot* dst,
                              const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                              int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride, uint32_t fields, uint64_t* keys_dev,
                              int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride, uint64_t* masks_dev, int64_t masks_stride, void* obs_dev,
                              int64_t obs_stride);

/* Trajectories that observe AgentMap views: the two calls above with the observation of ngw_snapshot_agent_view in the place of the lidar rows -
 * the egocentric window, the facing id and the inventory of the parent and of the state every step leaves.  `views` names the outputs, all device
 * memory, each recorded only where its pointer is not NULL (not all three NULL):
 *   view_dev    int8  [n_steps + 1][stride][W][W], W = 2 * view_size + 1: cell (i, k) of a window is map cell (r - view_size + i, c - view_size + k)
 *               of the state, (r, c) the agent's cell, 0 outside the map; the window is NOT rotated with the facing (the reference's get_agentView).
 *   facing_dev  int32 [n_steps + 1][stride]: the facing id.
 *   inv_dev     int32 [n_steps + 1][stride][K]: the inventory, K = the spec's item count.
 * Row numbering is the lidar rows': n_steps + 1 ROW BLOCKS of `stride` rows each, row j of block 0 is the parent of pair j, row j of block t + 1 the
 * state step t leaves, before any reset; every row is exactly what ngw_snapshot_agent_view returns for a slot holding that state.  All three are
 * all zeros for a step the pair did not execute (its episode is over, its limit is reached) and in every block - block 0 included - for a skipped
 * pair (NGW_F_BAD_INDEX).  One wavefront serves 64 consecutive pairs and stores its 64 rows of a block as one run of consecutive dwords: stride
 * must be a multiple of 64 and at least count rounded up to 64, view_dev 16-byte aligned (facing_dev, inv_dev: 4), and rows count .. of every block
 * (up to the next multiple of 64) are written with zeros; rows beyond that are not touched.  Offsets are 64-bit: the buffers may exceed 4 GiB.
 * view_size is in [1, NGW_TRAJ_VIEW_MAX].  obs_dev must be NULL: a call observes one kind.  ngw_lidar_configure is not needed, and nothing of the
 * lidar - configured or not, fused or not - is read or written.
 * Everything else - rewards, masks, limits, keys, reports, index rules, ordering, the stream, what is committed: nothing - is the _traj calls', which
 * are these calls with views == NULL.  One kernel launch (the same kernels: the view outputs are run-time arguments of the TRAJ forms); the windows
 * are built from the wavefront's 64 maps in LDS, no row leaves it.
 * Map sizes.  The launch runs under the handle's rollout layout - the path calls' layout - with the 64 * (K | 1) dwords of inventory shadows behind it
 *   only where keys_dev is set; the views need no LDS of their own.  So every handle the path calls serve is served - the Pogostick spec up to
 *   47 x 47, with keys too; with a fused int32 lidar of 8 beams (a larger layout of the handle's own) up to 45 x 45 without keys and 44 x 44 with
 *   them (45 x 45: 164 432 B) - while the lidar rows stop at 46 x 46 / 44 x 44 by their own layout.  A handle beyond it is refused: the message
 *   starts with "map_size" and names the bytes.
 * NGW_E_INVALID_ARG: what the _traj calls refuse; a NULL handle; views with all three pointers NULL; view_size outside [1, NGW_TRAJ_VIEW_MAX]; a stride
 * that is no multiple of 64 or below count rounded up to 64; a view_dev that is not 16-byte aligned; obs_dev and views both set; a layout that does
 * not fit LDS. */
#define NGW_TRAJ_VIEW_MAX 16
typedef struct ngw_traj_views {
    int32_t view_size;
    int8_t* view_dev;
    int32_t* facing_dev;
    int32_t* inv_dev;
    int64_t stride;
} ngw_traj_views;
int ngw_snapshot_rollout_traj_views(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride,
                                    int32_t n_steps, const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev,
                                    int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride,
                                    int32_t* rewards_dev, int64_t rewards_stride, void* obs_dev, int64_t obs_stride, const ngw_traj_views* views);
int ngw_snapshot_playout_traj_views(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed,
                                    uint64_t first_pair, const float* weights_dev /* NULL: the uniform rule */, const int32_t* limits_dev, ngw_snapshot* dst,
                                    const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                                    int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride, uint32_t fields, uint64_t* keys_dev,
                                    int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride, uint64_t* masks_dev, int64_t masks_stride, void* obs_dev,
                                    int64_t obs_stride, const ngw_traj_views* views);

/* Key table: an open-addressing hash set of 64-bit keys in device memory - "have I seen this state BEFORE?" across the calls of a search that
 * runs many iterations (transposition tables, duplicate removal in breadth-first solvers, Go-Explore archives, count-based bonuses).  A table
 * belongs to the handle that created it; it stores keys and nothing else (but see the valued tables below): a caller keeps what it wants per state (visit counts, the best return,
 * the archive slot) in arrays of its own of `buckets` entries, indexed by `where`.
 *   buckets  the smallest power of two >= 2 * capacity (not stored in the ABI: compute it); capacity in [1, 2^29].
 *   insert   for j < count: where[j] (int32) = the bucket that holds keys[j], and fresh[j] (uint8, 0 / 1) = 1 exactly when keys[j] was not in the
 *            table before this call AND j is the smallest position of this call that holds that key.  `fresh` is deterministic: it does not depend
 *            on the order in which the device runs the keys.  Equal keys get equal `where`, in this call and in every later one until the table is
 *            cleared; different keys get different `where`; every value lies in [0, buckets).  WHICH bucket a key gets is not part of the contract:
 *            it may depend on races between different keys that collide.
 *   lookup   where[j] = the bucket that holds keys[j], or -1 when the table does not hold it.  It changes nothing.
 *   count    *n = the number of keys in the table (a stream-ordered copy of a device counter; waits for the stream).
 *   clear    empties the table.
 * Key 0 is never stored: it is the empty-bucket mark, and what ngw_state_keys returns for a bad index (which has raised NGW_F_BAD_INDEX already).
 * For key 0, where = -1 and fresh = 0, and no flag is raised.
 * There is no probe limit short of the table: a key that finds neither itself nor a free bucket after probing EVERY bucket is refused - where = -1,
 * fresh = 0, and the sticky NGW_F_TABLE_FULL (ngw_error_flags) is raised; a refusal therefore means that all `buckets` buckets are occupied.
 * keys_dev (uint64 [count]), where_dev (int32 [count]) and fresh_dev (uint8 [count]) are DEVICE memory; exactly [0 .. count) of each output is
 * written.  count == 0 is a no-op.  Insert is two kernel launches (ngw_table.inc: the probe, then `fresh` from the buckets' stamps), lookup one;
 * all are enqueued on the handle's stream and do not wait.  Every call of one table must run on the handle's stream in the order of the calls:
 * concurrent inserts into one table from two streams are not supported.  The calls write no env state: nothing is committed, every derived buffer
 * stays as current as it was, a captured graph stays valid.
 * ngw_key_table_destroy waits for the stream (queued calls may still use the table) and frees it; ngw_destroy frees what is still open.
 * NGW_E_INVALID_ARG: a NULL handle, table, keys or output; a table that is not an open table of this handle; capacity outside [1, 2^29]; count < 0. */
typedef struct ngw_key_table ngw_key_table;
int ngw_key_table_create(ngw_handle* h, int64_t capacity, ngw_key_table** out);
int ngw_key_table_destroy(ngw_handle* h, ngw_key_table* t);
int ngw_key_table_clear(ngw_handle* h, ngw_key_table* t);
int ngw_key_table_insert(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, int64_t count, int32_t* where_dev, uint8_t* fresh_dev);
int ngw_key_table_lookup(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, int64_t count, int32_t* where_dev);
int ngw_key_table_count(ngw_handle* h, ngw_key_table* t, int64_t* n);

/* Valued key tables: the table also keeps, per key, the SMALLEST int32 value ever offered with it and an int32 tag stored by the offer that brought
 * that value - "is this the best way I have found to this state?" for uniform-cost, A* and label-correcting searches, and Go-Explore archives that
 * keep the better trajectory into a cell; with tags that name the parent, the way back to the root (ngw_key_table_trace).
 *   create_valued  as ngw_key_table_create, and the table holds a value and a tag per bucket: NGW_VALUE_NONE (never valued) and NGW_TAG_ROOT until
 *            an offer stores others.  A table of ngw_key_table_create holds neither, and insert_min / read / trace refuse it.  first_sequence (at
 *            most 2^62) is where the table's position counter starts (and starts again after a clear); EVERY result of every call is the same for
 *            every value of it - it exists so that a test can place the renormalising pass below where it wants it.
 *   insert_min     an insert that also offers values.  where[j] and fresh[j] are exactly what ngw_key_table_insert stores for the same keys: the same
 *            buckets, the same stamps, the same NGW_F_TABLE_FULL, the same treatment of key 0.  For a key k let before(k) be the value the table held
 *            for it before the call (NGW_VALUE_NONE if k was absent or never valued), and the call's OFFER for k the position with the smallest
 *            (values[j], j) among the positions j with keys[j] = k, where[j] >= 0 and values[j] != NGW_VALUE_NONE.  Then
 *                best[j] (uint8, 0 / 1) = 1  exactly when j is that offer AND values[j] < before(k)
 *            - strictly: an equal value of a later call is no improvement -, afterwards the table holds min(before(k), values[offer]) for k, and where
 *            best[j] = 1 and tags_dev != NULL it holds tags[j] as k's tag (otherwise the tag stays).  A position whose value is NGW_VALUE_NONE makes
 *            no offer: it behaves as under ngw_key_table_insert (best = 0).  Every other int32 is an ordinary value: negative ones, INT32_MIN.  `best`
 *            is deterministic: it depends neither on the order in which the device runs the positions nor on which bucket a key got.  At most one
 *            position per key and call has best = 1, so best - through ngw_frontier_compact - is the list of states to (re)open.
 *            count in [0, 2^31 - 1].  Two kernel launches, as insert; once per 2^32 positions offered to the table one more pass over its buckets.
 *   read     value[j], tag[j] = the value and the tag of bucket where[j] (what insert / insert_min / lookup reported).  A bucket of -1 or NGW_IDX_NONE
 *            gives (NGW_VALUE_NONE, NGW_TAG_ROOT); so does any other bucket outside [0, buckets), which also raises NGW_F_BAD_INDEX.  A bucket that
 *            holds no key, or a key never valued, reads as (NGW_VALUE_NONE, NGW_TAG_ROOT) too.  One kernel launch; it changes nothing.
 *   trace    reads the tags as tag = parent_bucket * n_actions + action and NGW_TAG_ROOT as "a root": for j < count, length[j] = the number of links
 *            from bucket where[j] to the first bucket on its chain whose tag is NGW_TAG_ROOT, root[j] = that bucket, and plans[t * count + j] (int32
 *            [steps][count], step-major: the layout ngw_snapshot_rollout takes) = the action of link t counted FROM THE ROOT for t < length[j], -1 for
 *            length[j] <= t < steps - the plan that leads from the root's state to the state of where[j], in execution order.  Tags are the caller's
 *            data and may form cycles, so at most `steps` links are followed: a chain that has not reached a root after `steps` links gives length =
 *            -1, root = -1 and a column of -1, and raises nothing.  where[j] of -1 or NGW_IDX_NONE gives the same, without a flag.  A bucket on the
 *            chain (where[j] included) outside [0, buckets) or without a key, or a tag other than NGW_TAG_ROOT outside [0, buckets * n_actions), gives
 *            the same and raises NGW_F_BAD_INDEX; no tag is used as an address before it is checked.  steps in [0, NGW_TRACE_MAX_STEPS], n_actions >=
 *            1 (the caller's convention, normally the spec's), buckets * n_actions <= 2^31 - 1, count in [0, 2^31 - 1].  One kernel launch, one lane
 *            per query; it changes nothing.
 * ngw_key_table_clear wipes values and tags with the keys; ngw_key_table_insert on a valued table leaves values and tags alone (a key it stores is
 * "never valued").  keys_dev / where_dev / fresh_dev as for insert; values_dev, tags_dev (int32 [count]; tags_dev may be NULL), best_dev (uint8
 * [count]), value_dev, tag_dev, length_dev, root_dev (int32 [count]) and plans_dev are DEVICE memory; exactly the entries named are written.  count
 * == 0 is a no-op.  All calls are enqueued on the handle's stream and do not wait; they write no env state.
 * NGW_E_INVALID_ARG: as for insert, and: a table without values; NULL values, best or outputs; first_sequence beyond 2^62; count, steps or n_actions
 * outside their ranges; buckets * n_actions > 2^31 - 1. */
#define NGW_VALUE_NONE INT32_MAX
#define NGW_TAG_ROOT (-1)
#define NGW_TRACE_MAX_STEPS 65536
int ngw_key_table_create_valued(ngw_handle* h, int64_t capacity, uint64_t first_sequence, ngw_key_table** out);
int ngw_key_table_insert_min(ngw_handle* h, ngw_key_table* t, const uint64_t* keys_dev, const int32_t* values_dev, const int32_t* tags_dev /* NULL: none */,
                             int64_t count, int32_t* where_dev, uint8_t* fresh_dev, uint8_t* best_dev);
int ngw_key_table_read(ngw_handle* h, ngw_key_table* t, const int32_t* where_dev, int64_t count, int32_t* value_dev, int32_t* tag_dev);
int ngw_key_table_trace(ngw_handle* h, ngw_key_table* t, const int32_t* where_dev, int64_t count, int32_t steps, int32_t n_actions, int32_t* plans_dev,
                        int32_t* length_dev, int32_t* root_dev);

/* Frontiers: the step `flags -> the index lists of the next call` of a search loop (expand -> keys -> insert -> next frontier), on the device.  The
 * number of hits stays in device memory: the lists have a fixed `capacity`, the live entries come first and NGW_IDX_NONE (above) pads the rest, so
 * the next call is launched at `capacity` and skips what is not there.  Nothing waits for the host, and a loop built on these two calls can be
 * enqueued ahead of time.
 * ngw_frontier_compact: let p_0 < p_1 < ... be the positions p in [0, n) with flags_dev[p] != 0 - ANY non-zero byte counts, 0x80 as well as 1 -,
 * total their number and taken = min(total, capacity).  Then
 *     first_dev[k]  (int32)            = map_dev ? map_dev[p_k / div] : p_k / div        for k < taken
 *     second_dev[k] (int32, or NULL)   = p_k % div                                       for k < taken
 *     first_dev[k] = second_dev[k]     = NGW_IDX_NONE                                    for taken <= k < capacity
 *     count_dev[0] = taken, count_dev[1] = total   (int32 [2])
 * and total > capacity raises the sticky NGW_F_FRONTIER_FULL.  The order is ascending and deterministic: the row-major order of a [rows, div] flag
 * array, so `first` is the row (through map_dev: the parent slot of that row) and `second` the column (the action).  Exactly [0, capacity) of the
 * lists and the two counts are written.  flags_dev (uint8 [n]) and map_dev (int32, at least ceil(n / div) entries, NULL: the identity) are DEVICE
 * memory and are only read; n in [0, 2^24], div >= 1, capacity in [0, 2^31 - 1].  n == 0 fills the lists with NGW_IDX_NONE and stores two zeros.
 * Two kernel launches (ngw_frontier.inc: the hits of every tile of 4096 flags, then the scatter), integer arithmetic only, no atomic orders the output.
 * ngw_frontier_alloc: let c = *cursor_dev and m = max(min(count_dev[0], limit - c), 0).  Then
 *     slots_dev[k] (int32) = c + k for k < m,  NGW_IDX_NONE for m <= k < capacity;     *cursor_dev = c + m afterwards
 * and m < count_dev[0] raises NGW_F_FRONTIER_FULL: a pool that is full degrades into dropped children - their pairs are skipped - and a flag, never
 * into a bad address.  count_dev is ngw_frontier_compact's (only [0] is read), cursor_dev an int32 in DEVICE memory that the caller initialises;
 * limit >= 0 is one past the last slot that may be handed out.  One kernel launch; the cursor is written after every work-group has read it.
 * Both are enqueued on the handle's stream and do not wait.  They write no env state: nothing is committed, a captured graph stays valid.
 * NGW_E_INVALID_ARG: a NULL handle, count or cursor, NULL flags with n > 0, a NULL list with capacity > 0; n outside [0, 2^24]; div < 1; capacity or
 * limit negative, capacity beyond 2^31 - 1. */
int ngw_frontier_compact(ngw_handle* h, const uint8_t* flags_dev, int64_t n, int32_t div, const int32_t* map_dev, int64_t capacity, int32_t* first_dev,
                         int32_t* second_dev, int32_t* count_dev);
int ngw_frontier_alloc(ngw_handle* h, const int32_t* count_dev, int32_t* cursor_dev, int32_t limit, int64_t capacity, int32_t* slots_dev);

/* Priority frontiers: the step "of these candidates, go on with the best k" - beam search, A*, best-first search over an archive, Go-Explore's
 * choice of cells - in the list form of ngw_frontier_compact, with no host wait.
 * ngw_frontier_select: values_dev (int32 [n]) is read as `groups` groups of m = n / groups values, group g the positions [g m, (g + 1) m).  A
 * CANDIDATE is a position p with values_dev[p] != NGW_VALUE_NONE - in both modes - and (flags_dev == NULL or flags_dev[p] != 0; any non-zero byte
 * counts, as in ngw_frontier_compact).  The candidates of a group are ordered by (value ascending, position ascending) when largest == 0 and by
 * (value descending, position ascending) when largest == 1, and the first taken_g = min(candidates_g, keep) of them are CHOSEN: at equal values the
 * smaller position wins, so the choice is a function of the inputs alone, whatever order the device runs in.  Let p_0 < p_1 < ... be the chosen
 * positions of group g in ASCENDING POSITION order (the row-major order of the compaction, not the order of the values).  Then
 *     first_dev[g keep + i]  (int32)          = map_dev ? map_dev[p_i / div] : p_i / div     for i < taken_g
 *     second_dev[g keep + i] (int32, or NULL) = p_i % div                                    for i < taken_g
 *     every other entry of [0, capacity) of both lists = NGW_IDX_NONE  (the rest of each group's span of `keep` entries, and [groups keep, capacity))
 *     taken_dev[g] (int32 [groups]) = taken_g
 *     bound_dev[g] (int32 [groups]) = the value of the last chosen candidate in selection order - the largest chosen value when largest == 0, the
 *                                     smallest when largest == 1 -, NGW_VALUE_NONE where taken_g == 0
 *     count_dev[1] = the candidates of all groups;  count_dev[0] = taken_0 when groups == 1 - the live entries are then a prefix and
 *                    ngw_frontier_alloc serves exactly them -, groups * keep when groups > 1: the live entries are no prefix there, the allocation hands
 *                    a slot to every entry of the spans and the call that takes the lists skips the padded pairs
 * No flag is raised: dropping what lies beyond `keep` is what the call is for.  values_dev, flags_dev (uint8 [n]) and map_dev (int32, at least
 * ceil(n / div) entries, NULL: the identity) are DEVICE memory and are only read; exactly [0, capacity) of the lists, the `groups` entries of
 * taken_dev and bound_dev and the two counts are written.  n in [0, 2^24], groups in [1, 2^24] with n a multiple of it, div >= 1, keep in
 * [0, 2^31 - 1] with groups * keep <= capacity, capacity in [0, 2^31 - 1], largest 0 or 1.  n == 0 (so m == 0) fills the lists with NGW_IDX_NONE,
 * taken with 0 and bound with NGW_VALUE_NONE; keep == 0 does the same, and count_dev[1] is still the number of candidates.
 * m <= 1024: one kernel launch, a wavefront per group; above: six launches behind a memset of the handle's scratch (ngw_select.inc).  Integer
 * arithmetic only; the entry of a chosen position comes from counts, no atomic orders the output.  Enqueued on the handle's stream, no wait, no
 * env state written.
 * NGW_E_INVALID_ARG: a NULL handle, taken, bound or count, NULL values with n > 0, a NULL first with capacity > 0; n outside [0, 2^24]; groups outside
 * [1, 2^24] or no divisor of n; div < 1; keep negative; groups * keep > capacity; capacity outside [0, 2^31 - 1]; largest neither 0 nor 1. */
int ngw_frontier_select(ngw_handle* h, const int32_t* values_dev, const uint8_t* flags_dev /* NULL: every position */, int64_t n, int32_t groups, int32_t div,
                        const int32_t* map_dev /* NULL: the identity */, int32_t keep, int32_t largest, int64_t capacity, int32_t* first_dev,
                        int32_t* second_dev /* NULL: not wanted */, int32_t* taken_dev, int32_t* bound_dev, int32_t* count_dev);

/* Search runs: whole best-first iterations over one snapshot pool and one valued key table, enqueued from ONE call with no host wait in between - the
 * label-correcting loop built from ngw_successor_keys, ngw_key_table_insert_min, ngw_frontier_compact / _select, ngw_frontier_alloc and
 * ngw_snapshot_expand as a library object, which also keeps the cost and the bucket every slot was reached with and the cheapest goal reached.
 * With A = the spec's n_actions, a search of `capacity` over `pool` and `table` owns, in DEVICE memory (ngw_search_arrays): two parent lists int32
 * [capacity] that take turns - the current frontier, NGW_IDX_NONE-padded -, g and bucket int32 [pool's capacity] - NGW_VALUE_NONE / -1 until a slot is
 * reached -, the cursor of its slot allocation int32 [1] (0 at creation; the caller sets it to the first free slot of the pool), and scratch of
 * capacity * A entries per array.  ngw_search_run allocates nothing.
 * cost(a, w), the cost of action a whose step reports the info word w: costs[a] when the search was created with by_action != 0, else
 * costs[NGW_INFO_COST(w)]; the table of 64 int32 is the caller's (the step costs scaled and rounded, or any other).
 *   start    the roots roots[0 .. count) (slots of the pool, DEVICE memory, count <= capacity, NGW_IDX_NONE allowed: skipped): their keys under
 *            NGW_KEY_STATE offered to the table by ngw_key_table_insert_min with value 0 and tag NGW_TAG_ROOT; then g[roots[j]] = the value the table
 *            holds for that key, bucket[roots[j]] = its bucket, and the current parent list becomes: roots[j] where best[j] was set - the first
 *            position of a state the table did not hold at 0 or below -, NGW_IDX_NONE elsewhere and behind `count`.
 *   run      `iterations` times, in this order, with P the current parent list and N the other one:
 *            1. ngw_successor_keys of P under NGW_KEY_STATE: keys and info words [capacity][A]; position q = j * A + a.
 *            2. offer: values[q] = g[P[j]] + cost(a, info[q]), tags[q] = bucket[P[j]] * A + a.  A padded parent (NGW_IDX_NONE, or any slot outside
 *               the pool), a parent whose g is NGW_VALUE_NONE, and a sum that would reach or pass NGW_VALUE_NONE (or fall below INT32_MIN) offer
 *               NGW_VALUE_NONE - no offer - and never wrap; the last case is counted (ngw_search_report: overflow, overflowed).
 *            3. ngw_key_table_insert_min(keys, values, tags): where, fresh, best.
 *            4. judge: a position with best[q] set whose info word has NGW_INFO_DONE set and a message code other than 14 (a FireWall death) is a
 *               goal reached more cheaply: the search's goal word is lowered to the smallest (values[q], where[q]) pair - ordered by value, then by
 *               bucket; a bucket holds one key, so the result does not depend on the order the device runs in.  With stop_at_goals, best[q] is
 *               then cleared wherever NGW_INFO_DONE is set, goal or death: an ended state is stored and valued but never expanded.
 *            5. keep < 0: ngw_frontier_compact(best, div = A); keep >= 0: ngw_frontier_select(values, flags = best, one group, keep, smallest first,
 *               div = A); both without a map: entries (j, a).  Then ngw_frontier_alloc on the search's cursor with limit = the pool's capacity.
 *            6. settle: for every entry k with a slot c = slots[k]: the expand lists (P[j], a, c); g[c] = values[j * A + a], bucket[c] = where[j * A +
 *               a], N[k] = c.  An entry without a slot (a full pool) keeps its pair with child NGW_IDX_NONE - skipped by the expand - and N[k] =
 *               NGW_IDX_NONE; padded entries stay NGW_IDX_NONE and write nothing.
 *            7. ngw_snapshot_expand(pool, the lists, pool), launched at `capacity`.  N becomes the current list.
 *            An iteration whose frontier is empty runs the same launches; they leave early.  NGW_F_FRONTIER_FULL, NGW_F_TABLE_FULL and
 *            NGW_F_BAD_INDEX are raised exactly where the five calls raise them; the three kernels raise none.  Every launch is enqueued on the
 *            handle's stream; nothing waits.  Nothing is committed: no env state, mask, lookahead table or mirror changes, a captured graph stays valid.
 *   read     waits for the stream: the iterations run, the goal (NGW_VALUE_NONE, -1 while none was reached), the cursor, the handle's sticky flags
 *            and, for the last `rows` = min(iterations, 64) iterations, oldest first, offered (positions that made an offer) / improved (best set by
 *            insert_min) / expanded (children written) / overflow.
 * `current` (may be NULL) receives which of the two parent lists is the current one.
 * NGW_E_INVALID_ARG: a NULL argument; a pool or table that is not open on this handle (also when it was closed since the creation); a table without
 * values; capacity outside [1, the pool's capacity] or capacity * A beyond 2^24; keep > capacity; buckets * A > 2^31 - 1 (a tag would not fit); maps
 * beyond ngw_successor_keys' limit; count outside [0, capacity]; iterations < 0. */
typedef struct ngw_search ngw_search;
typedef struct ngw_search_arrays {
    void* parents[2];
    void* g;
    void* bucket;
    void* cursor;
} ngw_search_arrays;
#define NGW_SEARCH_ROWS 64
typedef struct ngw_search_report {
    int64_t iterations;
    uint64_t overflowed;        /* offers dropped because the sum left the int32 range, over the whole search */
    int32_t goal_value, goal_bucket;
    int32_t cursor;
    uint32_t flags;             /* ngw_error_flags, read without clearing */
    int32_t rows, current;
    uint32_t stats[NGW_SEARCH_ROWS][4];   /* offered, improved, expanded, overflow */
} ngw_search_report;
int ngw_search_create(ngw_handle* h, ngw_snapshot* pool, ngw_key_table* table, int64_t capacity, const int32_t* costs_host /* [64] */, int32_t by_action,
                      int32_t keep /* < 0: every improved state */, int32_t stop_at_goals, ngw_search_arrays* arrays, ngw_search** out);
int ngw_search_destroy(ngw_handle* h, ngw_search* s);
int ngw_search_start(ngw_handle* h, ngw_search* s, const int32_t* roots_dev, int64_t count, int32_t* current);
int ngw_search_run(ngw_handle* h, ngw_search* s, int32_t iterations, int32_t* current);
int ngw_search_read(ngw_handle* h, ngw_search* s, ngw_search_report* out);

/* Open-list searches: the third discipline beside the layered (keep < 0) and the beam form (keep >= 0) of ngw_search_create.  A state that was reached
 * but not yet expanded stays a candidate of every later iteration, ordered by f = g + h: uniform-cost search (h = 0), A* (h from ngw_snapshot_walk),
 * "the most promising cell of the whole archive".  ngw_search_create_open makes the same ngw_search object - ngw_search_start / _run / _read / _destroy
 * serve it - which owns, beside the arrays above and in the same ONE allocation (ngw_search_arrays_open):
 *     h  int32 [pool's capacity]   the heuristic of the state in each slot; 0 until written
 *     f  int32 [pool's capacity]   the priority of each OPEN slot; NGW_VALUE_NONE for a slot that is unreached, closed (expanded, pruned or superseded)
 *                                  or never opened.  The library reads f only in the selection of step 0 and writes it only where stated below: a
 *                                  caller who runs one iteration at a time and rewrites f of the open slots (a learned value, say) gets that order.
 *     slot_of_bucket int32 [table's buckets], -1 at creation: the slot that holds the cheapest copy of the bucket's state
 * and the walk's distances [capacity][K], the selection's words and a second stats ring.  ngw_search_run allocates nothing in that allocation; the
 * selection of step 0 uses the handle's scratch as every ngw_frontier_select does, which grows - once, with a wait - at the first call over more
 * values than any selection on the handle before.  `keep` (1 <= keep <= capacity) is how many open states an
 * iteration expands, chosen from the WHOLE open list; `capacity` stays the width of the lists, so it bounds the children written per iteration: with
 * keep * A <= capacity no improved child is dropped by the compaction (beyond that NGW_F_FRONTIER_FULL reports the drop, as above).
 * The walk heuristic (heuristic = NGW_SEARCH_H_MIN or _MAX, weights_host: K = n_items int32 >= 0): with d = the K distances ngw_snapshot_walk gives a
 * slot, h(slot) = the minimum (_MIN: "walk to the nearest of these") or the maximum (_MAX: "all of these are needed") of int64(weights[k]) * d[k] over
 * the k with weights[k] > 0 and d[k] >= 0, clamped to NGW_VALUE_NONE - 1; 0 where there is no such k, and everywhere under NGW_SEARCH_H_NONE.
 * Whether h is admissible is the caller's business (rule of thumb: the weight is the cheapest of the three movement costs in the search's cost table).
 *   start    as above, and for each root taken (best[j] set): slot_of_bucket[its bucket] = the root, h[root] by the rule above, f[root] =
 *            min(int64(g[root]) + h[root], NGW_VALUE_NONE - 1).  The current parent list is then EMPTY (all NGW_IDX_NONE): the first iteration
 *            chooses the roots from the open list like any other state.  A second start adds its roots to what is there: the open list, h and
 *            slot_of_bucket stay as the iterations before left them, so a search is not restarted by clearing its table - destroy it and create
 *            another.
 *   run      an iteration, with P the current parent list and N the other one:
 *            0. SELECT: ngw_frontier_select(values = f, flags = NULL, n = the pool's capacity, one group, div = 1, no map, keep, smallest first,
 *               capacity): P = its `first` list, the chosen slots in ascending slot order, NGW_IDX_NONE behind them; ties in f go to the smaller
 *               slot.  TAKE, per entry: f[slot] = NGW_VALUE_NONE (closed); with prune, an old f >= the goal's value (none yet: NGW_VALUE_NONE)
 *               makes P[k] = NGW_IDX_NONE - valid for an admissible h and non-negative costs: such a state cannot lead to a cheaper goal.  Once
 *               a goal is known, iterations stop expanding what cannot beat it, and when nothing can they expand nothing (the launches leave
 *               early on empty lists): the early stop on the device.
 *            1. - 4. as above.
 *            5. ngw_frontier_compact(best, div = A) ALWAYS - the choice was made in step 0, every improved child is kept -, then ngw_frontier_alloc.
 *            6. settle as above, and SUPERSEDING: for a child written to slot c with bucket b, an earlier slot named by slot_of_bucket[b] gets f =
 *               NGW_VALUE_NONE - its state has been reached more cheaply, it is never expanded from the dearer copy - and is counted (whether it
 *               was still open or not); then slot_of_bucket[b] = c.  (best is set at most once per key and call: one writer per bucket.)
 *            7. ngw_snapshot_expand as above.  N becomes the current list: the children written by this iteration.  P - the slots this iteration
 *               expanded, NGW_IDX_NONE where pruned - stays in the other list (ngw_search_arrays.parents[1 - current]) until the next iteration
 *               makes it its N.
 *            8. OPEN: with a heuristic, ngw_snapshot_walk(pool, N, count = capacity, items = NULL, the distances) - a padded entry gives a row of -1
 *               and no flag -; then for every child c of N: h[c] by the rule above (0 without a heuristic), f[c] = min(int64(g[c]) + h[c],
 *               NGW_VALUE_NONE - 1).  A child that stop_at_goals barred never reached the list and is never opened.
 *            A slot written by anything but the search keeps f = NGW_VALUE_NONE and is never chosen.
 *   read_open  waits for the stream: for the last `rows` = min(iterations, 64) iterations, oldest first: chosen (slots the selection took), pruned,
 *            superseded, open (the candidates in the list before the choice: the selection's count[1]), f_min and f_bound (the smallest and the
 *            largest f chosen, pruned ones included; NGW_VALUE_NONE for an empty choice).  f_min is the minimum of the whole open list at the
 *            start of that iteration, so with an admissible h, a goal of value v and f_min >= v (or open == 0): C* >= f_min >= v >= C* - the goal
 *            is proven cheapest, provided no state was lost (no NGW_F_FRONTIER_FULL, no NGW_F_TABLE_FULL).
 * NGW_E_INVALID_ARG: what ngw_search_create refuses; keep < 1; a pool beyond 2^24 slots (the selection's limit); a heuristic mode other than the three;
 * n_weights != n_items, a NULL or a negative weight under a heuristic; ngw_search_read_open on a search made by ngw_search_create. */
#define NGW_SEARCH_H_NONE 0
#define NGW_SEARCH_H_MIN 1
#define NGW_SEARCH_H_MAX 2
typedef struct ngw_search_options {
    int64_t capacity;
    const int32_t* costs_host;      /* [64] */
    int32_t by_action, keep, stop_at_goals, prune;
    int32_t heuristic;              /* NGW_SEARCH_H_* */
    int32_t n_weights;              /* n_items under a heuristic */
    const int32_t* weights_host;    /* [n_weights]; not read under NGW_SEARCH_H_NONE */
} ngw_search_options;
typedef struct ngw_search_arrays_open {
    ngw_search_arrays base;
    void* h;
    void* f;
} ngw_search_arrays_open;
typedef struct ngw_search_open_report {
    int64_t iterations;
    int32_t rows, reserved;
    int32_t stats[NGW_SEARCH_ROWS][6];   /* chosen, pruned, superseded, open, f_min, f_bound */
} ngw_search_open_report;
int ngw_search_create_open(ngw_handle* h, ngw_snapshot* pool, ngw_key_table* table, const ngw_search_options* options, ngw_search_arrays_open* arrays,
                           ngw_search** out);
int ngw_search_read_open(ngw_handle* h, ngw_search* s, ngw_search_open_report* out);

/* The recipe heuristic: a lower bound on the craft / extract / break cost that a state still has to pay before it holds the goal item, read off its
 * inventory and - for tools that work from the map, the Pogostick tap - off the count of an item on its map.  The term beside the walk heuristic:
 * movement actions and rule actions are disjoint, so lower bounds on their costs add.  A relaxed plan over a PROGRAM the caller compiles from the
 * spec's recipe table and the search's cost table (search.recipe_program does; search.recipe_cost_reference states the evaluation in numpy).
 * A program holds the goal item, a bit mask `map_items` (bit k: cells of id k on the map count as held; at most NGW_RECIPE_MAX_MAP_ITEMS bits, none of
 * an item that a rule consumes) and n_rules <= NGW_RECIPE_MAX_RULES rules, each ONE successful application of one action:
 *     out_item, out_qty in [1, 65535], cost in [0, NGW_VALUE_NONE), n_in <= 4 inputs (in_item, in_qty in [1, 65535]) that it consumes, and tool_item
 *     (-1: none): an item that must be held, and is kept.
 * No two rules give the same item, and the order is topological, consumers first: a rule's inputs and its tool are given by LATER rules, if by any.
 * An item without a rule costs nothing to demand: the bound is weaker there, never wrong.
 * Evaluation, in integers:
 *     have[k] = inv[k] + (the cells of id k on the map, if bit k of map_items is set);   need[goal_item] = 1, every other need 0;   h = 0
 *     for each rule in order:   d = max(0, need[out_item] - have[out_item]);   n = ceil(d / out_qty);   h += n * cost;
 *                               need[in_item[i]] += n * in_qty[i];   if n > 0 and tool_item >= 0: need[tool_item] = max(need[tool_item], 1)
 * with every product and sum taken in 64 bits, need saturating at 2^31 - 1 and h at NGW_VALUE_NONE - 1.
 * ngw_snapshot_recipe_costs: out_dev[j] = h of row idx_dev[j] of `s` (NULL: the handle's current states; a NULL list: row j), count rows; one launch, no
 * LDS staging of maps - every map size -, and a program without map_items reads no map at all.  NGW_IDX_NONE gives 0 silently, an index out of range
 * 0 and NGW_F_BAD_INDEX.  Nothing is committed.
 * ngw_search_set_recipe: an open-list search adds the term - h = min(recipe + walk, NGW_VALUE_NONE - 1) for every root and every child opened; the
 * kernel runs once per ngw_search_start and once per iteration over the list the open step reads.  Legal only before the first ngw_search_start; the
 * scratch (one int32 per list entry) is allocated here, ngw_search_run still allocates nothing.  Without the call a search computes what it always did.
 * NGW_E_INVALID_ARG: a program that breaks a rule above; a search that is not an open-list one, or was started. */
#define NGW_RECIPE_MAX_RULES 16
#define NGW_RECIPE_MAX_INPUTS 4
#define NGW_RECIPE_MAX_MAP_ITEMS 4
typedef struct ngw_recipe_rule {
    int32_t out_item, out_qty, cost, n_in;
    int32_t in_item[NGW_RECIPE_MAX_INPUTS], in_qty[NGW_RECIPE_MAX_INPUTS];
    int32_t tool_item;              /* -1: none */
} ngw_recipe_rule;
typedef struct ngw_recipe_program {
    int32_t goal_item, n_rules;
    uint32_t map_items;
    int32_t reserved;
    ngw_recipe_rule rules[NGW_RECIPE_MAX_RULES];
} ngw_recipe_program;
int ngw_snapshot_recipe_costs(ngw_handle* h, ngw_snapshot* s /* NULL: the current states */, const int32_t* idx_dev, int64_t count,
                              const ngw_recipe_program* program, int32_t* out_dev);
int ngw_search_set_recipe(ngw_handle* h, ngw_search* s, const ngw_recipe_program* program);

/* Guided playouts: ngw_snapshot_playout_traj_views whose weights depend on the STATE - at every step the pair's current state is looked up in a key
 * table, and where the table holds it the choice is made under that bucket's row of the caller's weights.  The selection phase of MCTS (descend by
 * the tree's statistics while the node is in the tree), tabular Q / softmax policies, Go-Explore's "return, then explore" and playouts whose bias is
 * learned per state, in one launch in the place of a host loop of keys -> lookup -> gather -> sample -> one-step rollout.
 * The rule.  For a pair that is alive at step t (not skipped, t below its limit, no earlier step ended its episode):
 *   1. k = the key under `fields` of the state the pair is in before step t: what ngw_state_keys returns for that row - for t = 0 the parent's key, for
 *      t > 0 the entry of step t - 1 of the path keys.  One `fields` governs the recorded keys and the look-up; it must be a non-empty selection even
 *      where keys_dev is NULL.
 *   2. b = what ngw_key_table_lookup(table, k) returns: the bucket, or -1 (key 0 gives -1).
 *   3. outside == NGW_OUTSIDE_STOP and b < 0: the pair executes neither this step nor any later one, exactly as if limits[j] were t - it is not
 *      `ended`, its recorded actions from t on are -1, its key / reward / mask entries 0, and a kept child receives the state it is in.
 *   4. Otherwise the step's weights are row b of table_weights_dev (float32 [buckets][n_actions], row-major, buckets as ngw_key_table_create
 *      defines them) where b >= 0, else weights_dev ([n_actions]), else - weights_dev == NULL - the uniform rule of ngw_snapshot_playout.
 *   5. The choice is rules 3 - 6 of ngw_sample_actions on the playout's own mask word m and Philox word w (the stream, tag and counter of
 *      ngw_snapshot_playout): mass 0 falls back to the uniform rule on the same w.  A bad weight (negative, NaN, above 2^64) counts as 0 and raises
 *      NGW_F_BAD_WEIGHT if it lies in a row that a pair read for a step it executed; a bad weight in a row no executed step read raises nothing.
 * So with an empty table and NGW_OUTSIDE_DEFAULT the call computes, bit for bit, what the same call without a table computes, and with every row
 * equal to weights_dev what the weighted playout computes.  The draw depends on (seed, first_pair + j, t), the state, the table's contents and the
 * weights alone: a call split with first_pair gives the rows of the whole one.
 * Outputs beyond the trajectory playout's (device memory, each may be NULL):
 *   where_dev  int32 [n_steps][where_stride], where_stride >= count: b of every executed step; -1 where the state was not in the table and -1 for a
 *              step the pair did not execute (the recorded actions tell the two apart).  Exactly [t * where_stride, + count) of every row is written.
 *   depth_dev  int32 [count]: the number of leading executed steps with where >= 0 - how far the pair stayed inside the table.  0 for a skipped pair.
 * The table is only read: its contents, its count and every bucket stay what they were, and nothing is committed.  The call is enqueued on the
 * handle's stream behind the table's earlier calls; an insert into the table concurrent with it is not supported.  One kernel launch
 * (ngw_playout.inc, GUIDED: the running key of the path form is what is looked up; the rows are read in place, 2 * n_actions floats per pair and step).
 * Map sizes: the running key needs the inventory shadows whether or not keys_dev is set, so the limit is that of the trajectory call WITH keys under
 * the same observation kind.
 * NGW_E_INVALID_ARG: what ngw_snapshot_playout_traj_views refuses; a NULL table or table_weights_dev; a table that is not an open table of this
 * handle; fields == 0 or a bit outside NGW_KEY_ALL; where_stride < count with where_dev; an `outside` that is neither value. */
#define NGW_OUTSIDE_DEFAULT 0   /* a state the table does not hold draws by weights_dev (NULL: uniformly) */
#define NGW_OUTSIDE_STOP 1      /* a state the table does not hold ends the pair there: the leaf of a tree descent */
int ngw_snapshot_playout_guided(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                                const float* weights_dev /* NULL: the uniform rule */, const int32_t* limits_dev, ngw_snapshot* dst,
                                const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                                int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride, uint32_t fields, uint64_t* keys_dev,
                                int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride, uint64_t* masks_dev, int64_t masks_stride, void* obs_dev,
                                int64_t obs_stride, const ngw_traj_views* views /* NULL: no views */, ngw_key_table* table, const float* table_weights_dev,
                                int32_t* where_dev, int64_t where_stride, int32_t* depth_dev, int32_t outside);

/* Tree-search runs: whole MCTS iterations - descend, simulate, expand one node, back up, reweight - over one key table, enqueued from ONE call with
 * no host wait and no work of the caller in between: the Monte-Carlo twin of ngw_search_run.  A tree keeps, per bucket b of its table and action a,
 *   visits[b][a]   int32     returns[b][a]  int64     rows[b][a]  float32 (the table_weights of its guided playouts)     priors[b][a]  float32 (optional)
 * and mask_words[b] (uint64; 0: never learned), all in ONE device allocation with the recorded arrays of an iteration's playout (`playouts` pairs of
 * `steps` = T steps).  The statistics are INTEGERS so that every sum is an integer addition: the result of a backup does not depend on the order the
 * device runs the adds in, nor on how they are combined on the way - which float sums (index_add_) do.  Every byte below is a public contract;
 * tree.py states it in numpy.
 *   iteration `it` (a 64-bit count since ngw_tree_create or ngw_tree_clear), with the current root list R (count pairs, count <= playouts):
 *     1. ngw_snapshot_playout_guided(src, R, count, n_steps = T, seed, first_pair = it * playouts, weights_dev = the tree's default-policy weights or
 *        NULL, table, table_weights_dev = rows, outside = NGW_OUTSIDE_DEFAULT), recording actions, path keys under `fields`, rewards, mask words,
 *        where and depth (stride `playouts`), through that entry point, unchanged.  The draws depend on (seed, it, j, t) and the state alone, so
 *        ngw_tree_run(4, seed) and four calls of ngw_tree_run(1, seed) leave identical statistics for every key, and identical bytes everywhere the
 *        table gives the keys the same buckets (two tables need not: ngw_key_table_insert leaves the bucket of colliding keys open).
 *     2. leaf: d = depth[j].  1 <= d < length[j]: leaf_keys[j] = keys[d - 1][j] - the first state of the pair the table does not hold - and
 *        leaf_masks[j] = masks[d][j], the word the default policy's draw at that state was made under.  Otherwise no leaf: key 0, mask 0.  d = 0: the
 *        root is not in the table (never started, or refused by a full table): the pair neither grows nor backs up.
 *     3. expand: ngw_key_table_insert(leaf_keys) -> where_leaf, fresh, through that entry point.  where_leaf[j] >= 0: mask_words[where_leaf[j]] =
 *        leaf_masks[j] (a leaf mask is never 0; a word of 0 - a root that was skipped - is not stored); equal states write equal words, so the race is benign and the result deterministic.  The statistics of a fresh bucket are 0
 *        (ngw_tree_create and ngw_tree_clear zero them).  A full table raises NGW_F_TABLE_FULL from the insert, as always; that pair does not grow.
 *     4. back up, every-visit, undiscounted: the bucket of step t of pair j is e = where[t][j] for t < d, where_leaf[j] for t == d, none for t > d
 *        (steps beyond the leaf are the default policy's, even where the walk re-enters the table).  For every executed step t <= d with e >= 0
 *        and a = actions[t][j]: visits[e][a] += 1 and returns[e][a] += G_t, G_t = the sum of rewards[u][j] over u >= t (+ bootstrap[j] where
 *        ngw_tree_backup was given one), as an int32 and an int64 two's-complement addition.
 *     5. reweight every bucket b touched in 3 or 4 (every other row keeps its bytes; the rule applied to an untouched row gives the bytes it has):
 *        m = mask_words[b]; n_b = the sum of visits[b][.] in 64 bits; in IEEE binary32, every operation rounded to nearest even on its own, none
 *        fused, integers converted to binary32 round-to-nearest-even:
 *            q[a] = float(returns[b][a]) / float(visits[b][a]) where visits[b][a] > 0, else q_init
 *            u[a] = ((c * p[a]) * sqrt(float(n_b + 1))) / float(1 + visits[b][a])        score[a] = q[a] + u[a]
 *        p[a] = 1 without priors, else priors[b][a] cleaned by rule 3 of ngw_sample_actions (outside [2^-64, 2^64]: +0; negative, NaN or above 2^64
 *        raises NGW_F_BAD_WEIGHT, valid action or not).  The row is 1.0f at the action chosen by: pick = none; for a = 0 .. A-1 in order: bit a of m
 *        set and (pick is none or score[a] > score[pick]) -> pick = a - the valid action of the largest score, the lowest id on ties -, 0.0f
 *        elsewhere; m == 0: an all-zero row, which the playout treats as the uniform rule.  A one-hot row on a valid action makes rules 3 - 6 of
 *        ngw_sample_actions pick that action with certainty, for every Philox word: v is 0 before it, so the first a with v[a] > 0 and c[a] = 1 >
 *        thr is it, and thr = u * 1 < 1 always - also in the corner w = 0, where thr = 0 and the comparison c[a] > thr is strict.
 *   create   the checks, the allocation (zero-filled) and the default-policy weights (weights_host: NULL or n_actions float32, copied).
 *   arrays   the device pointers: the statistics (the caller reads them and fills priors) and the recorded arrays of the last iteration.  Waits for the
 *            stream once, so that what the caller then writes (priors) cannot be overtaken by the allocation's zero-fill.
 *   start    the roots: slots of `src` (NULL: the envs' current states), DEVICE memory, count <= playouts, NGW_IDX_NONE allowed (skipped).  Their keys
 *            under `fields` (ngw_state_keys) are inserted, their mask words learned - the word ngw_sample_actions reports for the row: rule 1's m -,
 *            and their rows written by rule 5.  visits and returns of a state the table already held are kept: re-rooting after a committed step
 *            keeps the statistics.  R becomes these roots.
 *   run      `iterations` iterations.  It allocates nothing, waits for nothing, and looks the table and the source up in the handle's lists before
 *            every iteration.
 *   grow / backup / reweight   the stages on their own, over the caller's arrays of a guided playout (step-major, stride `stride`, n_steps <= T, count
 *            <= playouts): grow = 2 and 3 (the leaves stay in the tree's where_leaf); backup = 4 with e of step d taken from where_leaf when
 *            use_leaves != 0 (else no pair has a leaf) and an optional int32 bootstrap [count]; reweight = 5 for a list of buckets (NULL: the buckets
 *            the last backup touched; -1 and NGW_IDX_NONE entries are skipped, any other entry outside [0, buckets) too).  They count nothing into
 *            the report and do not advance `it`.
 *   report   waits for the stream: the iterations run, the handle's sticky flags (not cleared) and, for the last `rows` = min(iterations, 64)
 *            iterations, oldest first: pairs alive (length >= 1), nodes grown (fresh), insertions refused (a leaf key without a bucket), steps backed
 *            up, the largest depth.
 *   clear    ngw_key_table_clear, the statistics, mask words, rows and the report zeroed, `it` = 0, no roots.  ngw_key_table_clear alone does NOT
 *            clear the statistics: the buckets' rows then describe keys the table no longer holds.  priors are the caller's and stay.
 * Nothing is committed, as for the guided playout.  Every launch is enqueued on the handle's stream.  A tree is rank-local.
 * NGW_E_INVALID_ARG: a NULL argument; a table (or a source) that is not open on this handle, also when it was closed since; playouts < 1, steps < 1,
 * playouts * steps > 2^31 - 1; buckets * n_actions > 2^31 - 1; fields == 0 or a bit outside NGW_KEY_ALL; c or q_init not finite; maps beyond the keyed
 * guided playout's limit (its message, "map_size ..."); count outside [0, playouts]; n_steps outside [1, steps]; stride < count; iterations < 0. */
typedef struct ngw_tree ngw_tree;
typedef struct ngw_tree_options {
    int64_t playouts;
    int32_t steps;
    uint32_t fields;
    float c, q_init;
    int32_t priors;                 /* != 0: the tree holds priors[buckets][A] (zero-filled: fill them before they are read) */
    int32_t plain_backup;           /* != 0: the backup adds lane by lane, without combining inside the wave (the same bytes; for A/B timing) */
    const float* weights_host;      /* NULL: states outside the table draw uniformly */
} ngw_tree_options;
typedef struct ngw_tree_device_arrays {
    void *visits, *returns, *mask_words, *rows, *priors;      /* priors NULL without them */
    void *roots, *actions, *keys, *rewards, *masks, *where, *depth, *length, *ret, *ended, *info;
    void *leaf_keys, *leaf_masks, *where_leaf, *fresh, *touched;
    int64_t buckets;
    int32_t n_actions, reserved;
} ngw_tree_device_arrays;
#define NGW_TREE_ROWS 64
typedef struct ngw_tree_report_rows {
    uint64_t iterations;
    uint32_t flags;
    int32_t rows;
    uint32_t stats[NGW_TREE_ROWS][5];   /* alive, grown, refused, backed up, largest depth */
} ngw_tree_report_rows;
int ngw_tree_create(ngw_handle* h, ngw_key_table* table, const ngw_tree_options* options, ngw_tree** out);
int ngw_tree_destroy(ngw_handle* h, ngw_tree* t);
int ngw_tree_arrays(ngw_handle* h, ngw_tree* t, ngw_tree_device_arrays* out);
int ngw_tree_start(ngw_handle* h, ngw_tree* t, ngw_snapshot* src /* NULL: the current states */, const int32_t* roots_dev, int64_t count);
int ngw_tree_run(ngw_handle* h, ngw_tree* t, int32_t iterations, uint64_t seed);
int ngw_tree_grow(ngw_handle* h, ngw_tree* t, const int32_t* depth_dev, const int32_t* length_dev, const uint64_t* keys_dev, const uint64_t* masks_dev,
                  int64_t stride, int64_t count, int32_t n_steps);
int ngw_tree_backup(ngw_handle* h, ngw_tree* t, const int32_t* actions_dev, const int32_t* rewards_dev, const int32_t* where_dev, const int32_t* depth_dev,
                    const int32_t* length_dev, int64_t stride, int64_t count, int32_t n_steps, int32_t use_leaves, const int32_t* bootstrap_dev);
int ngw_tree_reweight(ngw_handle* h, ngw_tree* t, const int32_t* buckets_dev /* NULL: what the last backup touched */, int64_t count);
int ngw_tree_report(ngw_handle* h, ngw_tree* t, ngw_tree_report_rows* out);
int ngw_tree_clear(ngw_handle* h, ngw_tree* t);
/* The rule of a tree (additive: a tree whose rule was never set enqueues what it always did and leaves the same bytes).
 *   spread = S in [1, 64], default 1 - rule 5 generalised.  The row of a touched bucket b with m = mask_words[b] != 0 is the allotment that S
 *     successive PUCT choices with virtual visits make:
 *         k[a] = 0 for all a;  n_b = the sum of visits[b][.] in 64 bits
 *         for i = 0 .. S-1:  root_i = sqrt(float(n_b + 1 + i))
 *                            q[a] as in rule 5 (virtual visits do not change q)      u[a] = ((c * p[a]) * root_i) / float(1 + visits[b][a] + k[a])
 *                            pick = rule 5's ordered walk over a = 0 .. A-1 on score[a] = q[a] + u[a];  k[pick] += 1
 *         rows[b][a] = float(k[a])
 *     in binary32, every operation rounded on its own, none fused, the integer sums formed in 64 bits and converted round-to-nearest-even; p cleaned
 *     and NGW_F_BAD_WEIGHT raised as in rule 5; m == 0: an all-zero row.  S = 1 gives rule 5's bytes.  The entries are small integers, so the running
 *     binary32 sum of ngw_sample_actions' rule over them is exact and its mass is S: pair j draws action a at a state with probability k[a] / S by
 *     its own (seed, pair, t) - the pairs of one root spread over the S choices inside the tree, and the playout is unchanged.  A score that is NaN
 *     (visits written negative by the caller) behaves as in the walk: it is never larger than the pick's, and is the pick only at the first valid action.
 *   discount_q16 = g in [0, 65536], default 65536 - rule 4 generalised.  len = length[j] clamped to [0, n_steps]; G_len = bootstrap[j] (0 without
 *     one) plus the rewards recorded at t >= len (a playout records 0 there); for t = len-1 .. 0: G_t = rewards[t][j] + D(G_{t+1}), D(x) = x for g ==
 *     65536 (no multiply) and otherwise (g * x) >> 16: the int64 two's-complement product, wrapping as int64 does, then an arithmetic right shift
 *     (floor, not truncation).  What is added where, and `touched`, are rule 4's.  Integers still: any combining gives the same bytes.  It holds for
 *     ngw_tree_backup too.
 *   rows16: which kernel writes the rows.  0: automatic - the one-lane kernel at spread 1, the 16-lane kernel (one list entry per 16 lanes, lane l
 *     holding the actions l, l + 16, l + 32; the visit sum and each round's pick reduced inside the row) above; 1: the 16-lane kernel also at spread
 *     1; 2: the one-lane kernel (spread 1 only).  The bytes are the same: the field exists to time the two forms against each other.
 * The rule is host state, read when a call is enqueued: it holds for everything enqueued after it until it is set again or the tree is destroyed;
 * ngw_tree_clear keeps it.  No kernel is launched, but the call DOES enqueue work on the handle's stream: one fill of `touched` with -1 (steps *
 * playouts * 4 bytes), which forgets the list of the last backup - ngw_tree_reweight(NULL) right after it rewrites no row, so rows are never
 * recomputed under a rule other than the one their backup ran under unless the caller names the buckets.  Set the rule once, not per iteration.
 * NGW_E_INVALID_ARG: a NULL argument, a tree or table not open on this handle, spread outside [1, 64], discount_q16 outside [0, 65536], rows16 outside
 * [0, 2], rows16 == 2 with spread > 1, reserved != 0. */
typedef struct ngw_tree_rule { int32_t spread; int32_t discount_q16; int32_t rows16; int32_t reserved; } ngw_tree_rule;
int ngw_tree_set_rule(ngw_handle* h, ngw_tree* t, const ngw_tree_rule* rule);

/* One-step lookahead tables: every action's outcome for every env, without taking a step.
 * For a handle with A = n_actions the table of the CURRENT state is three arrays - reward int32, done uint8, info uint32 (the NGW_INFO_* packing).
 * Entry (i, a) holds exactly what ngw_get_step_out would report for env i if ngw_step_device were called now with action a for that env, under
 * the handle's spec - every novelty, the wrapper predicates (FireWall death, FenceRestriction, Crate), the axe rules, Jump, Chop, the sticky
 * `done` with its forced reward - and under its autoreset setting: a step that reaches the horizon reports done = 1, and info bit 1 is set only
 * for goal-done.  Bit 0 of info[i][a] equals bit a of env i's action mask, by construction (one predicate).  Columns a >= n_actions do not exist.
 * Nothing is committed: after the call every byte of the state is what it was - map, pose, inventory, selected item, step_count, episode -, and so
 * are the last step's reward / done / info, the prepared next episodes, the mask buffer, the lidar rows, the bit rows and the host mirrors; no
 * reset is performed and no prepared row is consumed, even for entries that end an episode.
 * The handle tracks whether its table describes the current state exactly as it does for the mask buffer: every launch that changes the state
 * (step, host step, reset, ngw_set_state, snapshot restore, rollout, graph launch) makes it stale, as does a change of the autoreset setting, and
 * the next query recomputes it (one kernel launch); a query on a current table launches nothing.  The buffers are allocated on first use and freed
 * by ngw_destroy.
 *   ngw_lookahead              makes the device table current (enqueued on the handle's stream; does not wait).
 *   ngw_get_lookahead          the table to host arrays [n_envs][A], env-major, made current first; any pointer may be NULL; waits for the stream.
 *                              A one-env handle whose resident step loop is running answers from the outcomes the loop has speculated for every
 *                              action of the current state: no launch, the loop keeps running.
 *   ngw_lookahead_device_ptrs  the device buffers in place (call ngw_lookahead before reading them; any pointer may be NULL).  The device layout
 *                              is ACTION-MAJOR, [A][n_pad] with n_pad = n_envs rounded up to a multiple of 64: entry (i, a) of each array is element
 *                              i * env_stride + a * action_stride (strides in ELEMENTS of the array's type; env_stride = 1, action_stride = n_pad),
 *                              so that one lane per env stores consecutive addresses.  Columns of padding envs are 0. */
int ngw_lookahead(ngw_handle* h);
int ngw_get_lookahead(ngw_handle* h, int32_t* reward, uint8_t* done, uint32_t* info);
int ngw_lookahead_device_ptrs(ngw_handle* h, void** reward, void** done, void** info, int64_t* env_stride, int64_t* action_stride);

/* Plan evaluation: what P candidate action sequences of T steps would return from the CURRENT state, without committing a step (the inner loop
 * of random-shooting / CEM planning, beam search, tree-search rollouts, scoring macro-actions).
 * Input: plans_dev, int32 in device memory; the action of env i, plan p, step t is plans_dev[(t * n_plans + p) * env_stride + i], env_stride >=
 * n_envs - the [T, N] row form of ngw_rollout_actions with a plan axis in the middle.
 * Plan p of env i is stepped from env i's current state on a private copy, by exactly the rules ngw_step_device applies: the handle's spec, every
 * novelty and wrapper predicate, its autoreset setting and horizon.  It STOPS at the first step that ends the episode, i.e. the first step whose
 * `done` (ngw_get_step_out) would be 1: the goal (including the sticky done of an env that already holds the goal item, autoreset off), a FireWall
 * death, the horizon under autoreset.  That step counts and its reward is included; later steps of the plan are not executed and add nothing.  No
 * reset runs.  Per (i, p):
 *   ret     int32   sum of the executed steps' rewards
 *   length  int32   number of steps executed, 1 .. n_steps
 *   ended   uint8   1 if the plan stopped at an episode end
 *   info    uint32  the NGW_INFO_* word of the last executed step (bit 1: goal-done, clear for a horizon cut; message code 14: FireWall death)
 * An action id outside [0, n_actions) behaves as in ngw_rollout_actions: that step leaves the private state untouched, contributes reward 0, counts
 * in `length`, its info word is 0, and the sticky NGW_F_INVALID_ACTION is raised.  With n_steps = 1, column p equals column a of the one-step
 * lookahead table for plans[0][p][i] = a.
 * Nothing is committed (the lookahead's list holds here too): every byte of the state, the last step's reward / done / info, the prepared next
 * episodes, the mask buffer and the lookahead table and whether they are current, the lidar rows, the bit rows, the host mirrors, the rollout
 * output rows and episode accumulators of ngw_rollout_outputs and the terminal-capture side set are what they were.  Because no reset runs, the call
 * is allowed while terminal capture is on.  A handle whose maps do not fit LDS (the fused rollouts' limit) refuses it.
 *   ngw_plan_eval              one kernel launch, enqueued on the handle's stream; does not wait.  Every call evaluates (there is no cached result).
 *   ngw_get_plan_eval          the results of the last evaluation to host arrays [n_envs][n_plans], env-major; any pointer may be NULL; waits.
 *   ngw_plan_eval_device_ptrs  the device buffers in place (any pointer may be NULL).  The device layout is PLAN-MAJOR, [n_plans][n_pad]: result
 *                              (i, p) of each array is element i * env_stride + p * plan_stride (strides in ELEMENTS; env_stride = 1, plan_stride
 *                              = n_pad), so that one lane per env stores consecutive addresses.  Columns of padding envs are 0.  The buffers (17 B per
 *                              pair) are allocated on first use, regrown - the pointers change - when a call brings more plans than any before, and
 *                              freed by ngw_destroy.
 * NGW_E_INVALID_ARG: NULL handle or plans, n_plans < 1, n_steps < 1, env_stride < n_envs, n_plans * n_pad beyond 32 bits, the two getters before any
 * evaluation, maps that do not fit LDS. */
int ngw_plan_eval(ngw_handle* h, const int32_t* plans_dev, int64_t env_stride, int32_t n_plans, int32_t n_steps);
int ngw_get_plan_eval(ngw_handle* h, int32_t* ret, int32_t* length, uint8_t* ended, uint32_t* info);
int ngw_plan_eval_device_ptrs(ngw_handle* h, void** ret, void** length, void** ended, void** info, int64_t* env_stride, int64_t* plan_stride);

#ifdef __cplusplus
}
#endif
#endif /* NGW_H */
