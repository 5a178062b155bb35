// ngw_host.h - internals shared by the translation units of the C-ABI's host side (ngw_abi_*.cpp).  Not installed, not part of include/ngw.h.
//   ngw_abi_create.cpp   spec checks, allocation and layout of a handle (state slab, LDS carve-ups, the HBM spec blob), small accessors
//   ngw_abi_launch.cpp   which kernel a call runs: steps, resets, rollouts, prepared next episodes and their cadence, hipGraph capture
//   ngw_abi_host.cpp     the host API's wire formats (ngw_step_host, ngw_step_host_packed), state in / out, the multi-GPU payload
//   ngw_abi_obs.cpp      observation wrappers on the device: LidarInFront (marches and the bit-row form), AgentMap
//   ngw_abi_debug.cpp    timing pair and diagnostics entry points (not in include/ngw.h)
//   ngw_abi_mask.cpp     action masks: the standalone mask kernel, staleness, the one-env loop's speculated records
//   ngw_abi_lookahead.cpp one-step lookahead tables: the lookahead kernel (ngw_lookahead.inc), staleness, the one-env loop's speculated records
//   ngw_abi_plans.cpp    plan evaluation: candidate action sequences scored from the current state without committing a step (ngw_plans.inc)
//   ngw_abi_snapshot.cpp device-side snapshots: save / restore / fork env states by index (ngw_snapshot.inc), expand saved states into new slots (ngw_expand.inc),
//                        roll action sequences out from saved states (ngw_slot_rollout.inc), observe saved states by slot (ngw_slot_observe.inc),
//                        64-bit state keys of saved slots and live envs (ngw_keys.inc), walk distances and go-to plans of them (ngw_walk.inc)
//   ngw_abi_table.cpp    device-side key tables: a hash set of such keys that outlives the call - insert, lookup, count, clear -, and a value and a tag per key: insert_min, read, trace (ngw_table.inc)
//   ngw_abi_frontier.cpp device-side frontiers: flags compacted into index lists of fixed capacity, slots handed out for them (ngw_frontier.inc),
//                        the k best candidates per group in the same list form (ngw_select.inc)
//   ngw_abi_search.cpp   search runs: the driver that enqueues whole best-first iterations - the five stages above through their own entry points, the three
//                        kernels of ngw_search.inc between them
//   ngw_abi_recipe.cpp   the recipe heuristic (ngw_recipe.inc): program checks, the launch, ngw_snapshot_recipe_costs
//   ngw_abi_tree.cpp     tree-search runs: the ngw_tree_* entry points and the driver that enqueues whole MCTS iterations - the guided playout and the
//                        table's insert through their own entry points, the six kernels of ngw_tree.inc between them
//
// Three rules hold in all of them:
//   1. Guard first.  An entry point that uses the handle's stream or its device state starts with `if (int rc = enter(h)) return rc;`
//      (current device, then the one-env handle's resident loop ended: HBM holds the state only once it has, and its stream is busy until
//      then), or reaches a helper that does (launch, rollout_chunks).  The entry points that deliberately do something else say why where
//      they do it (ngw_get_action_mask, ngw_action_mask_device_ptr, ngw_step_host, ngw_create); tests/test_solo_stop_audit.py checks it.
//   2. Whoever writes the state in HBM says so through state_written().  The handle carries facts DERIVED from that state - the host
//      mirrors, the delta shadows, the action masks, the occupancy bit rows - and state_written() is the one place that knows which of them
//      a write leaves behind (the lookahead table is one more of them).  A path assigns one of those flags itself only where it has just made the thing valid again.
//   3. Nothing is passed to launch() through the handle.  What one launch needs beyond its positional arguments travels in a LaunchOpts;
//      the handle holds what outlives the call.
#ifndef NGW_HOST_H
#define NGW_HOST_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/ngw.h"
#include "ngw_device.h"

namespace ngwh {
int fail(int code, const char* fmt, ...);           // sets the thread-local message ngw_last_error() returns; returns `code`
const char* last_error();
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return ngwh::fail(NGW_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define D2H(dst, src, bytes)                                                                             \
    do {                                                                                                 \
        if (dst) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDefault, h->stream));        \
    } while (0)
#define H2D(dst, src, bytes)                                                                             \
    do {                                                                                                 \
        if (src) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDefault, h->stream));        \
    } while (0)

// A device-side snapshot (ngw_abi_snapshot.cpp): `cap` rows of the seven state arrays in ONE allocation of its handle.
struct ngw_snapshot {
    int64_t cap = 0;
    void* slab = nullptr;
    int memcpy_path = 0;                  // NGW_SNAP_MEMCPY=1 when it was created: a save / restore without index lists runs as seven device-to-device copies instead of the kernel (A/B)
    NgwSnapRows r{};
};

// A device-side key table (ngw_abi_table.cpp): key[buckets] | stamp[buckets] | the counter of stored keys, in ONE allocation of its handle; a
// valued table (ngw_key_table_create_valued) holds best[buckets] (64-bit words) | tag[buckets] (int32) behind the counter in the same allocation.
struct ngw_key_table {
    int64_t cap = 0;
    uint64_t buckets = 0;                 // the smallest power of two >= 2 * cap
    uint64_t* slab = nullptr;
    uint64_t base = 0;                    // first + keys ever offered since the last clear (+ what insert_min skipped to keep the low half from wrapping): the stamp of position j of an insert is base + j
    uint64_t first = 0;                   // where base starts: first_sequence of ngw_key_table_create_valued, else 0
    uint64_t epoch = 0;                   // a valued table: the high half of the positions whose low halves the words of best[] carry (insert_min renormalises when base has left it)
    bool valued = false;
};

// A search run (ngw_abi_search.cpp): the pool and the table it works on - looked up by address in the handle's lists before every use, never
// dereferenced first -, and ONE allocation of its handle that holds every array: the goal word and the overflow count, the keys, the int32 arrays
// (stats rows, cost table, cursor and counts, the lists, g and bucket, the per-position scratch, an open-list search's own) and the two flag arrays.
struct ngw_search {
    ngw_snapshot* pool = nullptr;
    ngw_key_table* table = nullptr;
    int64_t cap = 0, pool_cap = 0, n = 0;   // n = cap * A positions
    int32_t A = 0, by_action = 0, keep = -1, stop = 0;
    int cur = 0;                          // which parent list is the current one
    int64_t iterations = 0;
    uint64_t* slab = nullptr;
    unsigned long long* goal = nullptr;   // slab[0]; slab[1]: the offers dropped at the int32 range
    uint64_t* keys = nullptr;             // [n]
    uint32_t* stats = nullptr;            // [NGW_SEARCH_ROWS + 1][4], row i % (NGW_SEARCH_ROWS + 1): iteration i (the spare row: the next iteration's, zero-filled ahead)
    int32_t *lut = nullptr, *cursor = nullptr, *count = nullptr, *taken = nullptr, *bound = nullptr;
    int32_t* parents[2] = {nullptr, nullptr};
    int32_t *first = nullptr, *second = nullptr, *slots = nullptr, *plist = nullptr, *g = nullptr, *bucket = nullptr;
    int32_t *info = nullptr, *values = nullptr, *tags = nullptr, *where = nullptr;
    uint8_t *fresh = nullptr, *best = nullptr;
    // an open-list search (ngw_search_create_open), in the same allocation: f, h [pool_cap], slot_of_bucket [buckets], the K weights and the walk's
    // distances [cap][K] (both start on 16 bytes; a search without a heuristic has neither), and the second stats ring
    bool open = false;
    int32_t prune = 0, hmode = 0, K = 0;
    int64_t buckets = 0;
    int32_t *f = nullptr, *h = nullptr, *slot_of_bucket = nullptr, *weights = nullptr, *dist = nullptr;
    uint32_t* ostats = nullptr;           // [NGW_SEARCH_ROWS + 1][NGW_SEARCH_OPEN_COLS], rows as in `stats`
    // the recipe term (ngw_search_set_recipe): the program and the term of every list entry [cap] - an allocation of its own, made by that call;
    // recipe NULL: no term, and every kernel gets what it got before there was one
    bool started = false;                 // ngw_search_start was called
    int32_t* recipe = nullptr;
    NgwRecipeProg recipe_prog{};
};

// A tree-search run (ngw_abi_tree.cpp): the table it keeps statistics for and the source of its roots - looked up by address in the handle's lists
// before every use, never dereferenced first -, and ONE allocation of its handle that holds every array: the statistics per bucket, the recorded
// arrays of an iteration's playout, the leaves and the stats ring.
struct ngw_tree {
    ngw_key_table* table = nullptr;
    ngw_snapshot* src = nullptr;          // where the roots live (ngw_tree_start); NULL: the envs' current states
    int64_t cap = 0, buckets = 0, n_roots = 0;   // cap: playouts per iteration
    int32_t T = 0, A = 0, combine = 1;
    int32_t spread = 1, discount_q16 = 65536, rows16 = 0;   // ngw_tree_set_rule; kept by clear
    uint32_t fields = 0;
    float c = 0, q_init = 0;
    uint64_t iterations = 0;              // since creation or the last clear
    uint64_t* slab = nullptr;
    unsigned long long* returns = nullptr;                      // [buckets][A]
    uint64_t *mask_words = nullptr, *keys = nullptr, *masks = nullptr, *leaf_keys = nullptr, *leaf_masks = nullptr;
    int32_t *visits = nullptr, *actions = nullptr, *rewards = nullptr, *where = nullptr, *touched = nullptr;
    int32_t *depth = nullptr, *length = nullptr, *ret = nullptr, *first_action = nullptr, *where_leaf = nullptr, *roots = nullptr, *start_actions = nullptr;
    uint32_t *info = nullptr, *stats = nullptr;   // stats: [NGW_TREE_ROWS + 1][NGW_TREE_COLS], rows as in ngw_search
    float *rows = nullptr, *priors = nullptr, *zero_weights = nullptr, *weights = nullptr;   // zero_weights [A][cap]: never written; weights [A]: the default policy's, or NULL
    uint8_t *ended = nullptr, *fresh = nullptr;
};

struct ngw_handle {
    ngw_spec spec;
    int64_t n = 0, n_pad = 0, env_base = 0;
    int device = 0;
    uint64_t seed = 0;
    int autoreset = 0, horizon = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    NgwBufs b{};
    NgwLaunch proto{};           // layout fields filled once
    size_t lds_bytes = 0;
    int map_mode = 0;
    NgwDevSpec* dspec = nullptr;      // LUT blob in HBM
    int32_t* actions_dev = nullptr;   // staging for host actions
    uint8_t* mask_dev = nullptr;
    uint32_t* info_host = nullptr;    // pinned staging of the packed info words (ngw_step_host)
    uint8_t* zc_host = nullptr;       // small batches: actions + packed outputs in host memory the GPU addresses directly
    uint8_t* zc_dev = nullptr;
    uint8_t* step_stage = nullptr;        // ngw_step_host, one-block layout: every output packed on the device, ONE copy out
    // ngw_step_host, delta refresh: device-side shadows of the map / inventory / selected rows the caller's block holds, the
    // block they describe (host pointer + its mapped device address), and whether it still mirrors the device state
    uint8_t* shadow[3] = {nullptr, nullptr, nullptr};
    const void* mirror_block = nullptr;
    uint8_t* mirror_dev = nullptr;
    bool mirror_valid = false;
    int wt_enabled = 1;                   // NGW_HOST_WRITE_THROUGH=0: the delta kernel behind every step instead of the step kernel's own stores into the block (A/B)
    bool shadow_stale = false;            // write-through steps ran since the shadows were seeded: the delta kernel needs them seeded again
    void* wt_block = nullptr;             // the block NgwDevSpec::wt points into
    uint32_t* wt_count = nullptr;         // device counter of finished blocks
    uint32_t wt_seq = 0;
    bool wt_rows = false;                 // NgwDevSpec::wt also points at the caller's lidar row buffer
    int host_delta = 1;                   // NGW_HOST_DELTA=0: every ngw_step_host copies the whole observation (A/B)
    size_t zc_bytes = (size_t)256 << 10;  // NGW_ZC_BYTES: largest ngw_step_host result written straight into mapped host memory (read at ngw_create)
    std::vector<void*> allocs;
    std::vector<void*> host_allocs;       // single-wavefront handles: the host mirror of the state (GPU-addressable page-locked memory)
    NgwMirror mir = {};                   // ... its arrays (host addresses = device addresses under unified addressing)
    uint8_t* mask_pin = nullptr; uint8_t* mask_pin_dev = nullptr;   // ngw_reset's mask: two page-locked halves the kernel reads in place
    hipEvent_t mask_ev[2] = {nullptr, nullptr};
    int mask_next = 0;
    uint8_t* act_pin_dev = nullptr;            // ... the same buffer as the GPU addresses it (ngw_step_host_packed: the kernel reads the actions in place)
    uint8_t* wire_stage = nullptr;             // ngw_step_host_packed: device staging of the dense sections
    uint8_t* act_pin = nullptr;                // ngw_step's actions: two page-locked halves feeding the asynchronous copy
    hipEvent_t act_ev[2] = {nullptr, nullptr};
    int act_next = 0;
    int hostres = 0;                         // single-wavefront handle with a host mirror (NgwMirror)
    uint32_t step_seq = 0;                   // hostres: sequence number of the last launch that reported one (LaunchOpts::seq)
    // ngw_step_host_packed, pipelined: the batch steps in slices on the handle's stream while a second stream brings the finished slices'
    // results across PCIe (api_slices: 0 / 1 = off - the default: measured slower, profiles/r05_ab.md -, NGW_API_SLICES=<n> selects n slices)
    hipStream_t stream2 = nullptr;
    hipEvent_t slice_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int api_slices = 0;
    // The one-env handle's resident step loop (ngw_solo.inc; NGW_SOLO=0 switches it off): a kernel that stays on the stream between the steps
    // of a host loop, speculates every action's outcome into `solo_out` and commits what the host posts into `solo_mbox`.
    int solo_enabled = 1;
    bool solo_running = false, solo_mirror_valid = false;
    uint32_t* solo_mbox = nullptr;            // page-locked, GPU-addressable: [0] command sequence, [1] action, [2] quit
    uint32_t* solo_out = nullptr;             // page-locked, GPU-addressable: [0] speculated sequence, [1] exited, records from dword NGW_SOLO_REC0
    uint32_t solo_seq = 0;                    // sequence number of the committed state as the host counts it
    int32_t solo_last_action = -1;            // the last action posted (re-posted to a fresh launch if the loop ended before it took it)
    NgwSolo solo_proto{};
    size_t solo_lds = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // timing pair
    hipEvent_t order_ev = nullptr;             // ngw_stream_order
    bool ev_marked = false;                    // ngw_timing_mark recorded the closing event already
    // LidarInFront observation
    NgwLidarDev* lidar_cfg = nullptr;     // device tables
    int32_t* lidar_out = nullptr;
    int lidar_len = 0, lidar_cap = 0;         // lidar_cap: row length lidar_out was allocated for
    int lidar_bits = 32;                  // row format of the lidar observation (ngw_lidar_set_output): 32 (the default: the reference's integers), 16 or 8 = packed
    int lidar_world = 0;                  // the ray table is one world-frame table rotated by the facing (NgwLidarDev::woff)
    uint8_t* lidar_host_rows = nullptr;   // ngw_lidar_host_rows: the packed host step also brings the observation rows across (the caller's page-locked buffer)
    NgwLaunch lidar_proto{};              // the stand-alone lidar launch: its own LDS layout
    // The O(1) lidar on occupancy bit rows (ngw_boards.inc).  lidar_boards: the configured ray table is the reference's default 8 beams and
    // the map is at most 32 x 32 (ngw_lidar_configure checks it entry by entry); boards_on: that, and the observation is fused - step launches
    // then run the in-place kernel with the bit-row epilogue, and whoever rewrites maps wholesale is followed by ngw_boards_kernel.
    int lidar_boards = 0;
    bool boards_on = false, brd_dirty = false;   // brd_dirty: the main set's bit rows do not describe its maps (ngw_set_state, a fused rollout): rebuilt before the next step launch
    NgwLaunch brd_proto{}, lb_proto{};    // launch layouts of ngw_boards_kernel / ngw_lidar_boards_kernel
    size_t brd_lds = 0, lb_lds = 0;
    int lidar_fused = 0, lidar_range = 0, lidar_beams = 0, lidar_chan = 0, lidar_ninv = 0;
    size_t lidar_lds = 0;
    NgwNx nx = {};                        // prepared next episodes (ngw_set_reset_prefetch); all null = off
    int prefetch_every = 0, since_refill = 0;
    // The cadence adapts under the DEFAULT setting: resets that find their prepared row stale (an env that ends two episodes
    // between refills - FireWall kills within a few steps) are counted on the device; the refill launch copies the count to a
    // host word and the host halves the cadence while it keeps growing, and doubles it back after four quiet refills.
    int cadence = 0, quiet = 0, noisy = 0, adapt = 1;
    int quiet_need = 4;                   // quiet refills before the cadence is doubled back (grows when a doubling had to be undone)
    bool probing = false;                 // the last change was a doubling
    uint32_t slow_seen = 0, refill_seen = 0, refill_count = 0;   // reports read / refill launches issued
    bool capturing = false;
    bool adapted = false;                 // adapt_cadence changed depth or cadence: a captured graph is stale (ngw_graph_launch re-captures it)
    bool adapt_error = false;             // growing the prepared-episode depth failed (out of memory): the depth stays, the next refill notes it once
    int prefetch_user = 0;                // the caller chose the cadence (ngw_set_reset_prefetch): ngw_set_autoreset leaves it alone
    int depth = 1, depth_user = 0;        // prepared episodes per env (power of two); depth_user: chosen through ngw_set_reset_prefetch_depth
    NgwTerm term = {};                    // terminal observations (ngw_set_terminal_capture); all null = off
    bool term_on = false;
    int32_t* row_reward = nullptr;        // fused rollouts: the caller's output rows (ngw_rollout_outputs)
    uint8_t* row_done = nullptr;
    int64_t row_stride = 0;
    int32_t* acc = nullptr;               // [4][n_pad] episode accumulators of the fused rollouts
    uint32_t off_rng = 0;                 // LDS dword offset of the reset path's Philox ring
    int fast_reset = 1;                   // dedicated new-episode kernel where it applies (NGW_FAST_RESET=0 / 2: the test suite's hook to run every reset through the general kernel / the dedicated one)
    NgwResetFast rf{};                    // its arguments, laid out once (layout_reset_fast)
    int rf_nw = -1, rf_additem = 0;       // rf_nw < 0: not applicable to this spec / layout
    size_t rf_lds = 0;
    int step_plain = 1;                   // NGW_STEP_PLAIN=0 (A/B): the general in-place kernel also where the plain instantiation applies
    uint64_t slab_span = 0;               // bytes from the state slab's base to the end of step_count, its last array the plain kernel addresses
    bool plain_class = false;             // the spec and the slab are in the plain class (ngw_step_plain_class, decided in ngw_create)
    bool last_step_plain = false;         // the last per-launch step ran the plain instantiation (ngw_step_kernel_info)
    int nostage = 0;                      // per-launch steps through the lean kernel without map staging (every size but 10 x 10 / 6 x 6; NGW_NOSTAGE=<min S*S>: A/B)
    NgwLaunch ns_proto{};                 // its launch prototype (small LDS layout)
    size_t ns_lds = 0;
    bool general_ok = true;               // false: the map is too big for the kernels that keep a wave's 64 maps in LDS (general kernel, fused rollouts, fused lidar)
    int ext = 0;                          // spec uses FireWall / FenceRestriction / Crate step predicates -> EXT kernels
    int8_t* view_out = nullptr;           // AgentMap windows
    int view_size = 0;
    size_t view_cap = 0;
    // The AgentMap window kept current (ngw_agent_view_fuse).  view_on: every committed step and reset leaves the windows of the state it produced in
    // view_out - built by the step kernel's VIEW form where the launch has one (view_fused, and view_size <= NGW_VIEW_FUSE_MAX), by the stand-alone
    // gather behind the launch everywhere else.  view_fresh: view_out describes the current state (state_written clears it; ngw_agent_view of the
    // same size then launches nothing).  A window of ANOTHER size asked for meanwhile goes to view_side and leaves view_out alone; view_last_side:
    // ngw_get_agent_view / ngw_agent_view_device_ptr hand out that one (the result of the last ngw_agent_view).
    bool view_on = false, view_fused = false, view_fresh = false, view_last_side = false;
    bool graph_view = false;              // the captured graph leaves the windows of the state it ends in
    int view_fuse_max = NGW_VIEW_FUSE_DEFAULT;   // largest view_size the step kernel builds itself (NGW_VIEW_FUSE, read by ngw_agent_view_fuse)
    int8_t* view_side = nullptr;
    int view_side_size = 0;
    size_t view_side_cap = 0;
    // Action masks (ngw_abi_mask.cpp, ngw_mask.inc): [n_pad] uint64 words in HBM.  act_mask_fresh: they describe the current state
    // (state_written clears it; a step with act_mask_on leaves the post-step masks behind it on the stream and sets it)
    uint64_t* act_mask = nullptr;
    bool act_mask_on = false, act_mask_fresh = false;
    bool graph_act_mask = false;          // the captured graph leaves the masks of the state it ends in
    int act_mask_fused = 1;               // NGW_MASK_FUSED=0: the standalone kernel behind every plain step instead of the fused form (A/B)
    // One-step lookahead table (ngw_abi_lookahead.cpp, ngw_lookahead.inc): action-major [n_actions][n_pad] reward / done / info in HBM, allocated on
    // first use.  look_fresh: nothing has written the state since it was computed (state_written ends that), under the autoreset setting
    // look_autoreset / look_horizon (a table computed under another setting than the handle's is recomputed too)
    int32_t* look_reward = nullptr;
    uint8_t* look_done = nullptr;
    uint32_t* look_info = nullptr;
    bool look_fresh = false;
    int look_autoreset = 0, look_horizon = 0;
    // Plan evaluation (ngw_abi_plans.cpp, ngw_plans.inc): plan-major [plan_cap][n_pad] return / length / ended / info in HBM, allocated on first use and
    // regrown when a call brings more plans.  plan_n: plans of the last evaluation (0 = none yet).  Not a fact derived from the state that anything
    // keeps current: every ngw_plan_eval runs the kernel.
    int32_t* plan_ret = nullptr;
    int32_t* plan_len = nullptr;
    uint8_t* plan_ended = nullptr;
    uint32_t* plan_info = nullptr;
    int32_t plan_cap = 0, plan_n = 0;
    int plan_major = 0;                   // NGW_PLAN_ORDER=plan when the buffers were first allocated: the plan-major block order (A/B, tools/plan_cost.py)
    std::vector<ngw_snapshot*> snaps;     // open snapshots (ngw_snapshot_create); their slabs are in `allocs`, ngw_destroy deletes what is left
    std::vector<ngw_key_table*> tables;   // open key tables (ngw_key_table_create); likewise
    std::vector<ngw_search*> searches;    // open search runs (ngw_search_create); likewise
    std::vector<ngw_tree*> trees;         // open tree-search runs (ngw_tree_create); likewise
    // Frontiers (ngw_abi_frontier.cpp): the scratch of ngw_frontier_compact / ngw_frontier_alloc, allocated on first use and regrown when a call
    // brings more tiles - word 0 the allocation's ticket (0 between the calls), the tile counts behind it
    int32_t* frontier_scratch = nullptr;
    int64_t frontier_tiles = 0;
    // ... and of ngw_frontier_select (ngw_device.h NgwSelect says what lies where), likewise
    uint32_t* select_scratch = nullptr;
    int64_t select_words = 0;
    long long solo_starts = 0;           // launches of the one-env resident loop (ngw_debug_solo_starts)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_steps = 0;
    bool graph_open = false;              // a SHORT graph (steps * 2 <= refill cadence) holds no refill: ngw_graph_launch keeps the cadence between its replays
    const int32_t* graph_actions = nullptr;   // what ngw_graph_build captured: an adaptation re-captures it
    int64_t graph_stride = 0;
};

namespace ngwh {

template <typename T>
int dev_alloc(ngw_handle* h, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = count * sizeof(T);
    HIP_TRY(hipMalloc(&q, bytes));
    HIP_TRY(hipMemsetAsync(q, 0, bytes, h->stream));
    h->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return NGW_OK;
}
void dev_free(ngw_handle* h, void* p);

// Is `p` still open on its handle?  `list` is one of the handle's four: snaps, tables, searches, trees.  Looked up by address, never dereferenced
// first: a closed object, or another handle's, is simply not found.
template <class T> bool is_open(const std::vector<T*>& list, const T* p) {
    for (const T* q : list)
        if (q == p) return true;
    return false;
}

// One description of a slab serves twice: run on a Carver without a base it only counts the bytes the allocation needs, run on the allocation it
// hands the arrays out - so the size and the offsets cannot disagree.  take() neither pads nor aligns: a description calls align() where it needs to.
struct Carver {
    char* base;
    size_t bytes = 0;
    explicit Carver(void* slab = nullptr) : base(static_cast<char*>(slab)) {}
    template <class T> T* take(size_t n) { const size_t at = bytes; bytes += n * sizeof(T); return base ? reinterpret_cast<T*>(base + at) : nullptr; }
    void align(size_t to) { bytes = (bytes + to - 1) / to * to; }
};

// Device tables of `rows` rows, n_pad elements apart (action-major, plan-major), to the caller's env-major out[n][rows] arrays: one strided copy
// per table brings the n live columns of every row across, ONE synchronisation waits for all of them, then the rows are transposed.  A table
// whose `out` is NULL is left alone.
struct RowTable { const void* dev; void* out; size_t elem; };   // elem: bytes per element, 1 or 4
inline int fetch_env_major(ngw_handle* h, int rows, std::initializer_list<RowTable> tables) {
    const size_t n = (size_t)h->n;
    std::vector<std::vector<uint8_t>> stage;
    for (const RowTable& t : tables) {
        stage.emplace_back(t.out ? n * (size_t)rows * t.elem : 0);
        if (t.out) HIP_TRY(hipMemcpy2DAsync(stage.back().data(), n * t.elem, t.dev, (size_t)h->n_pad * t.elem, n * t.elem, (size_t)rows, hipMemcpyDefault, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    auto transpose = [&](auto* out, const auto* src) {
        for (int r = 0; r < rows; r++)
            for (size_t i = 0; i < n; i++) out[i * (size_t)rows + (size_t)r] = src[(size_t)r * n + i];
    };
    size_t k = 0;
    for (const RowTable& t : tables) {
        const uint8_t* src = stage[k++].data();
        if (!t.out) continue;
        if (t.elem == 4) transpose(static_cast<uint32_t*>(t.out), reinterpret_cast<const uint32_t*>(src));
        else transpose(static_cast<uint8_t*>(t.out), src);
    }
    return NGW_OK;
}

// ngw_abi_create.cpp
void lidar_format(const ngw_handle* h, NgwLaunch& p);
int layout_lds(ngw_handle* h);
int upload_reset_u(ngw_handle* h);
void layout_reset_fast(ngw_handle* h);
// ngw_abi_launch.cpp
// What ONE launch() needs beyond its positional arguments; most calls pass the defaults.
struct LaunchOpts {
    enum Actions { ACT_I32 = 0, ACT_ARG = 1, ACT_U8 = 2 };   // (NgwLaunch::use_action0's values)
    Actions actions = ACT_I32;            // `actions_dev` holds int32 ids / is not read, the one env's action is `action0` / holds one byte per env
    int32_t action0 = 0;
    uint32_t seq = 0;                     // single-wavefront handles: the number the kernel reports to flags_host[NGW_SEQ_WORD] once the host mirror is written (0: neither)
    bool wire = false;                    // the step kernel's host write-through form (NgwWT); it reports h->wt_seq
    bool masks = true;                    // false: a step of a multi-step call that is not its last - its masks could never be read, none are computed
    int32_t* row_reward = nullptr;        // fused rollouts: this launch's first output rows (ngw_rollout_outputs) and the episode accumulators
    uint8_t* row_done = nullptr;
    int64_t row_stride = 0;
    int32_t* acc = nullptr;
};
int launch(ngw_handle* h, int mode, int n_steps, const int32_t* actions_dev, const uint8_t* mask_dev, uint64_t action_seed, int64_t t0,
           const LaunchOpts& o = LaunchOpts());
int launch_refill(ngw_handle* h);
int enter(ngw_handle* h);                           // rule 1: the handle's device made current, its one-env loop ended
enum : unsigned { WROTE_MAPS = 1u, WROTE_BY_SOLO_LOOP = 2u };
void state_written(ngw_handle* h, unsigned how = 0);   // rule 2
int ensure_boards(ngw_handle* h);                   // boards mode: the main set's bit rows rebuilt from its maps if they are stale
int refresh_fused_obs(ngw_handle* h);               // the fused LidarInFront observation of the state in HBM, as launches of its own
int steps_since_refill(ngw_handle* h, int k);       // prepared next episodes: k more steps' worth consumed; the refill launch when the cadence is reached
int solo_stop(ngw_handle* h);                       // ends the one-env handle's resident step loop (no-op when it is not running): what enter() does for every entry point
int solo_step(ngw_handle* h, int32_t action);      // one step() through the loop: the host mirror (h->mir) holds the new state afterwards
bool solo_ok(const ngw_handle* h);
int launch_step_slice(ngw_handle* h, const uint8_t* actions_u8_dev, int64_t first, int64_t count);   // one slice of a batched step (byte actions), on the handle's stream
int step_slices_done(ngw_handle* h);                // the bookkeeping of ONE batched step (refill cadence) once its slices are out
int publish_nx(ngw_handle* h, bool on);
int alloc_nx(ngw_handle* h, int depth, bool on);
void adapt_cadence(ngw_handle* h);
int rebuild_boards(ngw_handle* h, const int8_t* map, uint32_t* brd, int64_t rows);
int launch_lidar_boards(ngw_handle* h);            // boards mode: the LidarInFront observation of the current state from the bit rows, as its own launch
void drop_graph(ngw_handle* h);
// ngw_abi_obs.cpp
size_t lidar_layout(const ngw_handle* h, NgwLaunch& q);   // the stand-alone lidar launch's LDS carve-up into q (S, MS, KP and the row format set) -> its bytes, whatever they come to
// ngw_abi_mask.cpp
int launch_act_mask(ngw_handle* h);                 // the masks of the state in HBM, on the handle's stream (allocates the buffer on first use)
// ngw_abi_obs.cpp
int launch_view(ngw_handle* h);                     // the kept AgentMap windows (view_on) of the state in HBM, as the stand-alone gather on the handle's stream
bool view_in_step(const ngw_handle* h);             // ... or built by the in-place step kernel's VIEW form, where the launch is otherwise a plain one
int alloc_act_mask(ngw_handle* h);                  // the mask buffer, published to NgwDevSpec::amask (no-op once allocated)
bool solo_records_ready(ngw_handle* h);             // the one-env loop's speculated records belong to the host's state (waits for them like solo_step, never stops the loop)
// ngw_abi_snapshot.cpp
// where the rows a call reads live: a snapshot's slots, or (s == NULL) the state slab's envs.  Only behind is_open(): a closed snapshot is not dereferenced
struct Source { NgwSnapRows r; int64_t rows; const char* unit; };   // (unit: the word of the "from %lld %s" messages)
Source source_of(const ngw_handle* h, const ngw_snapshot* s);
// ngw_abi_recipe.cpp
// checks a program against the rules of include/ngw.h and the handle's K, and packs it for the kernel (ngw_device.h NgwRecipeProg)
int recipe_pack(const ngw_handle* h, const ngw_recipe_program* in, NgwRecipeProg* out);
// out_dev[j] = the cost of row idx_dev[j] of `src`: one launch on the handle's stream, for a caller that stands behind enter(); count > 0
int recipe_run(ngw_handle* h, const NgwSnapRows& src, int64_t rows, const int32_t* idx_dev, int64_t count, const NgwRecipeProg& prog, int32_t* out_dev);
// ngw_abi_host.cpp
void host_step_layout(const ngw_handle* h, uint64_t off[11]);
int check_actions(const int32_t* actions, size_t n, int A);   // NGW_E_INVALID_ACTION naming the first id outside [0, A)

// Which kernel an NGW_MODE_STEP launch runs: the in-place step kernel (no map staging) unless the fused lidar needs the maps in LDS for its march.
inline bool step_in_place(const ngw_handle* h) { return h->nostage && (!h->lidar_fused || h->boards_on); }
// ... and whether a launch of it takes the plain instantiation: the handle's class (spec and slab), the switch, and what the handle has switched on since
inline bool step_plain(const ngw_handle* h) { return h->plain_class && h->step_plain && step_in_place(h) && !h->ext && !h->boards_on; }

// The *_device_ptr(s) getters of buffers that are allocated on first use (action masks, the lookahead table): exempt from rule 1 - they end the
// one-env loop only if they have to allocate (the allocation zero-fills on the handle's stream); once the buffer exists they hand it out while the loop runs.
inline int enter_to_allocate(ngw_handle* h, bool allocated) {
    HIP_TRY(hipSetDevice(h->device));
    if (!allocated && h->solo_running) return solo_stop(h);
    return NGW_OK;
}

inline void cpu_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}

// Waits for a kernel's sequence number in host memory: polling the word costs a PCIe write's latency where a stream synchronisation costs
// several microseconds (and would also wait for a refill launch that follows on the stream).  Bounded: after `spins` polls without it the
// stream is synchronised the usual way.  The caller's reads of what the kernel wrote stay behind the wait.
inline int wait_seq(ngw_handle* h, volatile uint32_t* word, uint32_t seq, uint32_t spins) {
    bool seen = false;
    for (uint32_t spin = 0; spin < spins; spin++) {
        if (*word == seq) { seen = true; break; }
        cpu_pause();
    }
    if (!seen) HIP_TRY(hipStreamSynchronize(h->stream));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return NGW_OK;
}

}  // namespace ngwh
#endif
