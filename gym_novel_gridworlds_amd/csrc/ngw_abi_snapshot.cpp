// ngw_abi_snapshot.cpp - device-side snapshots (see ngw_host.h): buffers of saved env states and the one kernel (ngw_snapshot.inc) that moves
// rows between them and the state slab through index lists.  A restore changes the state behind the library's back-ups, so it reports it
// as ngw_set_state does (state_written), and then refreshes a fused lidar observation and schedules a refill of the prepared next
// episodes, as ngw_reset does.  A copy moves rows from slot to slot, inside one snapshot or between two, through the same kernel.  An expand (ngw_expand.inc) steps rows of the state slab or of a snapshot into slots of a snapshot: it commits
// nothing, so it neither calls state_written() nor touches anything the handle derives from its state, and counts no steps against the
// prepared-episode cadence (no reset runs).  A rollout (ngw_slot_rollout.inc) steps such rows through a whole action sequence and keeps the end
// state, the numbers, or both: it commits nothing either.  The slot observations (ngw_slot_observe.inc) read saved rows and write the caller's
// buffers: lidar rows, agent views, action masks of saved states.  They commit nothing, and leave the env's own observation buffers alone.
// The state keys (ngw_keys.inc) hash rows of a snapshot or of the state slab into the caller's buffer: they commit nothing either.
// The successor keys (ngw_successors.inc) are the keys of every action's child of such rows, with no child stored: they commit nothing either.
// A playout (ngw_playout.inc) is a rollout whose actions the kernel draws among the valid ones of each step: it commits nothing either.
// The path forms of both (ngw_path.inc) add per-pair step limits and the key of every visited state: they commit nothing either.
// The trajectory forms (ngw_traj.inc) add the per-step rewards, mask words and LidarInFront rows of such a path: they commit nothing either, and
// leave the env's own lidar rows alone.  Their AgentMap views (the _traj_views entry points) are outputs of the same launches under the path form's
// layout: no lidar is needed or touched.
// A guided playout (ngw_playout.inc, GUIDED) reads a key table and the caller's weight rows at every step: it commits nothing either, and leaves
// the table as it was.
// The weighted choice (ngw_sample.inc) draws one action per row by the caller's weights among the valid ones: it commits nothing either.
// The walk (ngw_walk.inc) finds the shortest Forward / Left / Right walks from such rows to each item id: it commits nothing either.
#include "ngw_host.h"

using namespace ngwh;

namespace {

NgwSnapRows state_rows(const ngw_handle* h) {
    NgwSnapRows r;
    r.map = h->b.map; r.loc = h->b.loc; r.facing = h->b.facing; r.inv = h->b.inv;
    r.selected = h->b.selected; r.step_count = h->b.step_count; r.episode = h->b.episode;
    return r;
}

}  // namespace

ngwh::Source ngwh::source_of(const ngw_handle* h, const ngw_snapshot* s) { return s ? Source{s->r, s->cap, "slots"} : Source{state_rows(h), h->n, "envs"}; }

namespace {

// `count` rows src -> dst on the handle's stream.  Without index lists the rows are contiguous: still the same kernel (one launch), or
// seven device-to-device copies when the snapshot was created under NGW_SNAP_MEMCPY=1 (the comparison: DESIGN.md 4.4).
int move_rows(ngw_handle* h, bool copies, const NgwSnapRows& src, int64_t src_rows, const int32_t* si, const NgwSnapRows& dst, int64_t dst_rows, const int32_t* di,
              int64_t count, bool keep_episode) {
    if (count == 0) return NGW_OK;
    const size_t S2 = (size_t)h->proto.S2, K = (size_t)h->proto.K, n = (size_t)count;
    if (copies && !si && !di) {
        HIP_TRY(hipMemcpyAsync(dst.map, src.map, n * S2, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dst.loc, src.loc, n * 8, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dst.facing, src.facing, n * 4, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dst.inv, src.inv, n * K * 4, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dst.selected, src.selected, n, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dst.step_count, src.step_count, n * 4, hipMemcpyDeviceToDevice, h->stream));
        if (!keep_episode) HIP_TRY(hipMemcpyAsync(dst.episode, src.episode, n * 4, hipMemcpyDeviceToDevice, h->stream));
        return NGW_OK;
    }
    NgwSnap a{};
    a.src = src; a.dst = dst; a.si = si; a.di = di; a.flags = h->b.flags;
    a.count = (int32_t)count; a.src_rows = (int32_t)src_rows; a.dst_rows = (int32_t)dst_rows;
    a.S2 = h->proto.S2; a.K = h->proto.K; a.keep_episode = keep_episode ? 1 : 0;
    HIP_TRY(ngw_snapshot_launch(&a, h->stream));
    return NGW_OK;
}

// a key selection; with `what`, also the stride of the [step][pair] keys a path or trajectory call writes
int key_args(uint32_t fields, const char* what = nullptr, int64_t count = 0, int64_t stride = 0) {
    if (!fields || (fields & ~NGW_KEY_ALL)) return fail(NGW_E_INVALID_ARG, "key fields 0x%x: a non-empty selection of NGW_KEY_* bits expected", (unsigned)fields);
    if (what && stride < count) return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with a key stride of %lld", what, (long long)count, (long long)stride);
    return NGW_OK;
}

// what the three slot observations check alike (before anything touches the stream)
int slot_obs_args(const ngw_handle* h, const ngw_snapshot* s, const void* out, const int32_t* slots_dev, int64_t count, const char* what) {
    if (!h || !s || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (count < 0 || count > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "%s of %lld slots", what, (long long)count);
    if (!slots_dev && count > s->cap) return fail(NGW_E_INVALID_ARG, "%s of %lld slots from a snapshot of %lld slots", what, (long long)count, (long long)s->cap);
    return NGW_OK;
}

// ... and fill alike
NgwSlotObs slot_obs(const ngw_handle* h, const ngw_snapshot* s, const int32_t* slots_dev, int64_t count) {
    NgwSlotObs x{};
    x.src = s->r; x.slots = slots_dev; x.flags = h->b.flags; x.count = (int32_t)count; x.rows = (int32_t)s->cap;
    return x;
}

// what an expand, a rollout and a playout check alike about their pairs (before anything touches the stream): where the parents live (-> from),
// where the children or end states go - count in [0, the destination's slots] -, and that the handle's maps fit the kernels' LDS layout.  A negative
// count is an expand's to refuse here (it has a destination); rollouts and playouts have refused it before.  what / call: "rollout", "ngw_snapshot_rollout"
int step_pairs_args(const ngw_handle* h, const ngw_snapshot* src, const int32_t* src_idx_dev, const ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count,
                    const char* what, const char* call, Source* from) {
    if (!dst && dst_slots_dev) return fail(NGW_E_INVALID_ARG, "destination slots without a destination snapshot");
    if ((dst && !is_open(h->snaps, dst)) || (src && !is_open(h->snaps, src))) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    *from = source_of(h, src);
    if (count < 0 || count > 0x7FFFFFFFll || (dst && count > dst->cap))
        return fail(NGW_E_INVALID_ARG, "%s of %lld states into a snapshot of %lld slots", what, (long long)count, (long long)(dst ? dst->cap : 0x7FFFFFFFll));
    if (!src_idx_dev && count > from->rows)
        return fail(NGW_E_INVALID_ARG, "%s of %lld states from %lld %s", what, (long long)count, (long long)from->rows, from->unit);
    if (!h->general_ok)
        return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps in LDS (%s, as the fused rollouts) "
                                       "and they need more than 160 KiB; per-launch steps and resets are available", h->proto.S, call);
    return NGW_OK;
}

// the launch block of the kernels that step saved rows: the handle's rollout layout - for an observing trajectory call the stand-alone lidar launch's
// layout and row format - with the handle's buffers, autoreset setting and horizon
NgwLaunch step_block(const ngw_handle* h, bool observing = false) {
    NgwLaunch a = observing ? h->lidar_proto : h->proto;
    a.b = h->b;
    if (observing) a.lout = nullptr;                 // (every tile goes to the caller's rows)
    a.autoreset = h->autoreset;
    a.horizon = h->horizon;
    return a;
}

// what the path forms ask for beyond a plain rollout / playout, and the trajectory forms beyond those (masks: playouts)
struct PathArgs { const int32_t* limits; uint32_t fields; uint64_t* keys; int64_t keys_stride; };
struct TrajArgs { int32_t* rewards; int64_t rewards_stride; uint64_t* masks; int64_t masks_stride; void* obs; int64_t obs_stride; NgwTrajViews vw; bool views; };
// where the actions come from: a plan [n_steps][stride], or the kernel draws them (weights NULL: the uniform rule; actions NULL: not recorded)
struct Plan { const int32_t* actions; int64_t stride; };
struct Draw { uint64_t seed, first_pair; const float* weights; int32_t* first_action; int32_t* actions; int64_t stride; };
// what a guided playout asks for beyond a trajectory playout: the table its states are looked up in, the [buckets][n_actions] weight rows, where the
// buckets and the depths go, and what a state outside the table does (include/ngw.h NGW_OUTSIDE_*)
struct GuideArgs { ngw_key_table* table; const float* rows; int32_t* where; int64_t where_stride; int32_t* depth; int32_t outside; };

// The one request behind the eight exported rollouts and playouts: step `count` pairs of saved rows up to n_steps times.  The form is the entry
// point's, never read off the pointers: a path call without limits and keys is still a path call.  The entry points fill it by member name.
enum Form { PLAIN, PATH, TRAJ };
struct Pairs {
    ngw_snapshot* src; const int32_t* src_idx;       // the parents: a snapshot's slots (NULL: the envs' current states), list NULL = 0 .. count-1
    ngw_snapshot* dst; const int32_t* dst_slots;     // where the end states go (NULL: nothing is kept)
    int64_t count; int32_t n_steps;
    int32_t* ret; int32_t* length; uint8_t* ended; uint32_t* info;   // the four reports, any may be NULL
    Form form; PathArgs pa; TrajArgs ta;             // (pa: PATH and TRAJ, ta: TRAJ; zeros otherwise)
    bool draws; Plan plan; Draw draw;                // (the one `draws` names; zeros otherwise)
    bool guided; GuideArgs ga;                       // (a TRAJ playout whose weights a key table chooses; zeros otherwise)
};

// the six launchers and the entry points they serve, by where the actions come from and by form
template <class X>
using PairsLaunch = hipError_t (*)(const NgwDevSpec*, const NgwLaunch*, const X*, int, size_t, hipStream_t);
const PairsLaunch<NgwSlotRollout> ROLLOUT_LAUNCH[3] = {ngw_slot_rollout_launch, ngw_slot_rollout_path_launch, ngw_slot_rollout_traj_launch};
const PairsLaunch<NgwPlayout> PLAYOUT_LAUNCH[3] = {ngw_playout_launch, ngw_playout_path_launch, ngw_playout_traj_launch};
const char* const PAIRS_CALL[2][3] = {{"ngw_snapshot_rollout", "ngw_snapshot_rollout_path", "ngw_snapshot_rollout_traj"},
                                      {"ngw_snapshot_playout", "ngw_snapshot_playout_path", "ngw_snapshot_playout_traj"}};
const char* const VIEWS_CALL[2] = {"ngw_snapshot_rollout_traj_views", "ngw_snapshot_playout_traj_views"};   // (TRAJ with a views struct)
const char* const GUIDED_CALL = "ngw_snapshot_playout_guided";                                                // (TRAJ with a table: views or not)

// The path and trajectory arguments of one request, checked (before anything touches the stream) -> the LDS bytes of the launch and where the
// inventory shadows sit.  Without observations: the path form's layout and its map limit.  With them: the stand-alone lidar launch's layout
// (ngw_lidar_configure), and the shadows behind it only where keys are asked for.  With AgentMap views: the handle's rollout layout as it is, and
// the shadows behind it only where keys are asked for - the views need no LDS of their own.  A guided playout keeps the running key whether or not
// keys are asked for: it has the shadows wherever a keyed call has them.
int path_traj_args(const ngw_handle* h, const Pairs& p, const char* what, const char* call, size_t* lds, uint32_t* off_shadow) {
    const PathArgs& pa = p.pa;
    const TrajArgs& ta = p.ta;
    const int64_t count = p.count;
    const bool shadows = pa.keys || p.guided;
    if (ta.rewards && ta.rewards_stride < count)
        return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with a reward stride of %lld", what, (long long)count, (long long)ta.rewards_stride);
    if (ta.masks && ta.masks_stride < count)
        return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with a mask stride of %lld", what, (long long)count, (long long)ta.masks_stride);
    if (pa.keys)
        if (int rc = key_args(pa.fields, what, count, pa.keys_stride)) return rc;
    if (ta.views) {
        const NgwTrajViews& v = ta.vw;
        if (!v.view && !v.facing && !v.inv) return fail(NGW_E_INVALID_ARG, "%s: views without a view, a facing and an inventory pointer: nothing to record", call);
        if (ta.obs) return fail(NGW_E_INVALID_ARG, "%s: lidar rows and views in one call; a call observes one kind", call);
        if (v.V < 1 || v.V > NGW_TRAJ_VIEW_MAX) return fail(NGW_E_INVALID_ARG, "view_size must be in 1..%d", NGW_TRAJ_VIEW_MAX);
        if (v.stride % NGW_EPB || v.stride < (count + NGW_EPB - 1) / NGW_EPB * NGW_EPB)
            return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with a view stride of %lld rows: a multiple of 64 that holds the pairs rounded up to 64 expected", what,
                        (long long)count, (long long)v.stride);
        if (reinterpret_cast<uintptr_t>(v.view) & 15u) return fail(NGW_E_INVALID_ARG, "%s: the view windows must be 16-byte aligned", what);
        if ((reinterpret_cast<uintptr_t>(v.facing) | reinterpret_cast<uintptr_t>(v.inv)) & 3u)
            return fail(NGW_E_INVALID_ARG, "%s: the facing ids and the inventories must be 4-byte aligned", what);
        *lds = h->lds_bytes + (shadows ? (size_t)NGW_EPB * 4u * (size_t)h->proto.KP : 0u);
        if (!h->general_ok)                          // (the handle kept no rollout layout: its maps and inventories alone are what can be named)
            return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps in LDS (%s) under the handle's rollout layout, whose maps and inventories "
                                           "alone take %zu B and which exceeds 160 KiB as a whole; per-launch steps with ngw_agent_view are available", h->proto.S, call,
                        (size_t)NGW_EPB * (size_t)h->proto.MS + (size_t)NGW_EPB * 4u * (size_t)h->proto.KP);
        if (*lds > NGW_PATH_LDS_MAX)
            return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps%s in LDS (%s) and they need %zu B, more than 160 KiB; %s", h->proto.S,
                        shadows ? " and a second copy of their inventories" : "", call, *lds,
                        shadows ? "the views without keys have the handle's own limit" : "per-launch steps with ngw_agent_view are available");
        return NGW_OK;
    }
    if (!ta.obs) {
        *lds = NGW_PATH_LDS_BYTES(h->lds_bytes, h->proto.KP);
        if (*lds > NGW_PATH_LDS_MAX)
            return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps and a second copy of their inventories in LDS (%s) and they need "
                                           "%zu B, more than 160 KiB; the plain call is available", h->proto.S, call, *lds);
        return NGW_OK;
    }
    if (!h->lidar_len) return fail(NGW_E_INVALID_ARG, "%s with observations before ngw_lidar_configure", call);
    if (ta.obs_stride % NGW_EPB || ta.obs_stride < (count + NGW_EPB - 1) / NGW_EPB * NGW_EPB)
        return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with an observation stride of %lld rows: a multiple of 64 that holds the pairs rounded up to 64 expected",
                    what, (long long)count, (long long)ta.obs_stride);
    if (reinterpret_cast<uintptr_t>(ta.obs) & 15u) return fail(NGW_E_INVALID_ARG, "%s: the observation rows must be 16-byte aligned", what);
    NgwLaunch q = h->proto;                          // (the size alone: a handle whose maps the lidar launch cannot hold has no lidar_proto)
    lidar_format(h, q);
    const size_t rows = lidar_layout(h, q);
    *off_shadow = (uint32_t)(rows / 4);
    *lds = rows + (shadows ? (size_t)NGW_EPB * 4u * (size_t)h->proto.KP : 0u);
    if (*lds > NGW_PATH_LDS_MAX || (h->general_ok && !h->lidar_lds))   // (general_ok == 0 with a layout that would fit: the plain refusal follows)
        return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps between two guards, the lidar tables and a tile of 64 observation rows%s in "
                                       "LDS (%s) and they need %zu B, more than 160 KiB; the call without observations %s", h->proto.S,
                    shadows ? " and a second copy of the inventories" : "", call, *lds, h->general_ok ? "has its own limit" : "is refused too");
    return NGW_OK;
}

// the caller's views struct into the request (NULL: the _traj call as it always was)
void views_arg(TrajArgs& ta, const ngw_traj_views* v) {
    if (!v) return;
    ta.views = true;
    ta.vw.view = v->view_dev; ta.vw.facing = v->facing_dev; ta.vw.inv = v->inv_dev; ta.vw.stride = v->stride; ta.vw.V = v->view_size;
}

// what NgwSlotRollout and NgwPlayout hold alike, out of the request
template <class X>
void fill_pairs(X& x, const Pairs& p, const Source& from, uint32_t off_shadow) {
    x.src = from.r; x.src_rows = (int32_t)from.rows; x.si = p.src_idx; x.di = p.dst_slots;
    if (p.dst) { x.dst = p.dst->r; x.dst_rows = (int32_t)p.dst->cap; x.keep = 1; }
    x.count = (int32_t)p.count; x.n_steps = p.n_steps;
    x.ret = p.ret; x.length = p.length; x.ended = p.ended; x.info = p.info;
    if (p.form != PLAIN) { x.limits = p.pa.limits; x.keys = p.pa.keys; x.keys_stride = p.pa.keys_stride; x.fields = p.pa.fields; x.off_shadow = off_shadow; }
    if (p.form == TRAJ) { x.rewards = p.ta.rewards; x.rewards_stride = p.ta.rewards_stride; x.obs = p.ta.obs; x.obs_stride = p.ta.obs_stride; }
    if (p.form == TRAJ && p.ta.views) x.vw = p.ta.vw;
}

// one request served: every check (in the order the entry points have always made them) before enter(h) and the first use of the stream, then one launch
int step_pairs(ngw_handle* h, const Pairs& p) {
    const char* const what = p.draws ? "playout" : "rollout";
    const char* const call = p.guided ? GUIDED_CALL : (p.ta.views ? VIEWS_CALL[p.draws] : PAIRS_CALL[p.draws][p.form]);
    const int64_t stride = p.draws ? p.draw.stride : p.plan.stride;
    if (!h || (!p.draws && !p.plan.actions)) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (p.n_steps < 1) return fail(NGW_E_INVALID_ARG, "%s of %d steps", what, (int)p.n_steps);
    if (p.count < 0 || ((!p.draws || p.draw.actions) && stride < p.count))
        return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with %s stride of %lld", what, (long long)p.count, p.draws ? "an action" : "a pair", (long long)stride);
    if (!p.draws && !p.dst && !p.ret && !p.length && !p.ended && !p.info && !p.pa.keys && !p.ta.rewards && !p.ta.obs && !p.ta.views)
        return fail(NGW_E_INVALID_ARG, "rollout without a destination and without a report: nothing to do");
    if (p.guided) {                                  // (the table and the rows: before anything touches the stream)
        const GuideArgs& g = p.ga;
        if (!g.table || !g.rows) return fail(NGW_E_INVALID_ARG, "NULL argument");
        if (!is_open(h->tables, g.table)) return fail(NGW_E_INVALID_ARG, "not an open key table of this handle");
        if (g.outside != NGW_OUTSIDE_DEFAULT && g.outside != NGW_OUTSIDE_STOP)
            return fail(NGW_E_INVALID_ARG, "outside %d: NGW_OUTSIDE_DEFAULT or NGW_OUTSIDE_STOP expected", (int)g.outside);
        if (g.table->buckets < 2 || g.table->buckets > (1ull << 30) || (g.table->buckets & (g.table->buckets - 1)))   // (what ngw_key_table_create makes; the kernel's bucket is an int32)
            return fail(NGW_E_INVALID_ARG, "%s: a key table of %llu buckets; a power of two in [2, 2^30] expected", GUIDED_CALL, (unsigned long long)g.table->buckets);
        if (int rc = key_args(p.pa.fields)) return rc;   // (the state that is looked up is named by `fields`, keys recorded or not)
        if (g.where && g.where_stride < p.count)
            return fail(NGW_E_INVALID_ARG, "%s of %lld pairs with a bucket stride of %lld", what, (long long)p.count, (long long)g.where_stride);
    }
    Source from;
    size_t lds = h->lds_bytes;
    uint32_t off_shadow = (uint32_t)(h->lds_bytes / 4);
    if (p.form == TRAJ)                              // (ahead of the plain refusal of large maps: this one names the bytes)
        if (int rc = path_traj_args(h, p, what, call, &lds, &off_shadow)) return rc;
    if (int rc = step_pairs_args(h, p.src, p.src_idx, p.dst, p.dst_slots, p.count, what, call, &from)) return rc;
    if (p.form == PATH)
        if (int rc = path_traj_args(h, p, what, call, &lds, &off_shadow)) return rc;
    if (int rc = enter(h)) return rc;
    if (p.count == 0) return NGW_OK;
    const NgwLaunch a = step_block(h, p.ta.obs != nullptr);
    if (!p.draws) {
        NgwSlotRollout x{};
        fill_pairs(x, p, from, off_shadow);
        x.actions = p.plan.actions; x.stride = p.plan.stride;
        HIP_TRY(ROLLOUT_LAUNCH[p.form](h->dspec, &a, &x, h->ext, lds, h->stream));
    } else {
        NgwPlayout x{};
        fill_pairs(x, p, from, off_shadow);
        x.actions = p.draw.actions; x.stride = p.draw.stride; x.first_action = p.draw.first_action;
        x.seed = p.draw.seed; x.first_pair = p.draw.first_pair; x.weights = p.draw.weights;
        if (p.form == TRAJ) { x.masks = p.ta.masks; x.masks_stride = p.ta.masks_stride; }
        if (p.guided) {
            const ngw_key_table* const t = p.ga.table;
            x.tkey = t->slab; x.tmask = t->buckets - 1; x.table_weights = p.ga.rows; x.tw_stride = h->spec.n_actions;
            x.where = p.ga.where; x.where_stride = p.ga.where_stride; x.depth = p.ga.depth; x.stop = p.ga.outside == NGW_OUTSIDE_STOP;
            HIP_TRY(ngw_playout_guided_launch(h->dspec, &a, &x, h->ext, lds, h->stream));
            return NGW_OK;
        }
        HIP_TRY(PLAYOUT_LAUNCH[p.form](h->dspec, &a, &x, h->ext, lds, h->stream));
    }
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_snapshot_create(ngw_handle* h, int64_t capacity, ngw_snapshot** out) {
    if (!h || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (capacity < 1 || capacity > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "snapshot capacity %lld outside [1, 2^31)", (long long)capacity);
    if (int rc = enter(h)) return rc;
    // one allocation, laid out like the state slab: every array 256-byte aligned, so a row is as aligned as its size allows
    const size_t cap = (size_t)capacity, S2 = (size_t)h->proto.S2, K = (size_t)h->proto.K;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_map = 0, o_inv = up(cap * S2), o_loc = o_inv + up(cap * K * 4), o_fac = o_loc + up(cap * 8), o_sel = o_fac + up(cap * 4),
                 o_stp = o_sel + up(cap), o_epi = o_stp + up(cap * 4), total = o_epi + up(cap * 4);
    uint8_t* slab = nullptr;
    if (int rc = dev_alloc(h, &slab, total)) return rc;               // (zero-filled on the handle's stream)
    ngw_snapshot* s = new ngw_snapshot;
    s->cap = capacity; s->slab = slab;
    if (const char* v = getenv("NGW_SNAP_MEMCPY")) s->memcpy_path = atoi(v) != 0;
    s->r.map = reinterpret_cast<int8_t*>(slab + o_map); s->r.inv = reinterpret_cast<int32_t*>(slab + o_inv);
    s->r.loc = reinterpret_cast<int32_t*>(slab + o_loc); s->r.facing = reinterpret_cast<int32_t*>(slab + o_fac);
    s->r.selected = slab + o_sel; s->r.step_count = reinterpret_cast<int32_t*>(slab + o_stp);
    s->r.episode = reinterpret_cast<uint32_t*>(slab + o_epi);
    // a never-saved slot is a legal state: an empty map with the agent at (1, 1)
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->r.loc), 1, cap * 2, h->stream);
    if (e != hipSuccess) {
        dev_free(h, slab);
        delete s;
        return fail(NGW_E_HIP, "hipMemsetD32Async failed: %s", hipGetErrorString(e));
    }
    h->snaps.push_back(s);
    *out = s;
    return NGW_OK;
}

int ngw_snapshot_destroy(ngw_handle* h, ngw_snapshot* s) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (int rc = enter(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                         // (queued saves / restores may still use the buffer)
    for (size_t i = 0; i < h->snaps.size(); i++)
        if (h->snaps[i] == s) { h->snaps.erase(h->snaps.begin() + (long)i); break; }
    dev_free(h, s->slab);
    delete s;
    return NGW_OK;
}

int ngw_snapshot_save(ngw_handle* h, ngw_snapshot* s, const int32_t* envs_dev, const int32_t* slots_dev, int64_t count) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (count < 0 || count > s->cap) return fail(NGW_E_INVALID_ARG, "save of %lld states into a snapshot of %lld slots", (long long)count, (long long)s->cap);
    if (!envs_dev && count > h->n) return fail(NGW_E_INVALID_ARG, "save of %lld states from %lld envs", (long long)count, (long long)h->n);
    if (int rc = enter(h)) return rc;
    return move_rows(h, s->memcpy_path != 0, state_rows(h), h->n, envs_dev, s->r, s->cap, slots_dev, count, false);
}

int ngw_snapshot_restore(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, const int32_t* envs_dev, int64_t count, int flags) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (count < 0 || count > h->n) return fail(NGW_E_INVALID_ARG, "restore of %lld states into %lld envs", (long long)count, (long long)h->n);
    if (!slots_dev && count > s->cap) return fail(NGW_E_INVALID_ARG, "restore of %lld states from a snapshot of %lld slots", (long long)count, (long long)s->cap);
    if (flags & ~NGW_SNAP_KEEP_EPISODE) return fail(NGW_E_INVALID_ARG, "unknown restore flags 0x%x", (unsigned)flags);
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    const bool keep = (flags & NGW_SNAP_KEEP_EPISODE) != 0;
    state_written(h, WROTE_MAPS);
    if (int rc = move_rows(h, s->memcpy_path != 0, s->r, s->cap, slots_dev, state_rows(h), h->n, envs_dev, count, keep)) return rc;
    // the fused observation of the restored state (what an explicit reset does as well): whole-batch launches however few envs were
    // restored - the price of an observation that is current right after the call
    if (int rc = refresh_fused_obs(h)) return rc;
    // Prepared next episodes: a row is valid iff its tag is the episode it was prepared for, so rows of envs whose counter moved are
    // merely stale (their next reset runs the placement loop: same result).  A refill behind the restore prepares fresh ones, like the
    // one behind an explicit reset; with the counters kept every tag still matches and nothing is scheduled.
    return keep ? NGW_OK : steps_since_refill(h, h->prefetch_every);
}

int ngw_snapshot_copy(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, ngw_snapshot* dst, const int32_t* dst_idx_dev, int64_t count) {
    if (!h || !src || !dst) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, src) || !is_open(h->snaps, dst)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (count < 0 || count > dst->cap) return fail(NGW_E_INVALID_ARG, "copy of %lld states into a snapshot of %lld slots", (long long)count, (long long)dst->cap);
    if (!src_idx_dev && count > src->cap) return fail(NGW_E_INVALID_ARG, "copy of %lld states from a snapshot of %lld slots", (long long)count, (long long)src->cap);
    if (src == dst && !src_idx_dev && !dst_idx_dev && count) return fail(NGW_E_INVALID_ARG, "copy of slots 0 .. %lld of a snapshot onto themselves", (long long)count - 1);
    if (int rc = enter(h)) return rc;
    // the whole row, the episode counter included; the plain copies only between two buffers (rows of one buffer go through the kernel, whose
    // pairs are disjoint by the call's contract)
    return move_rows(h, src != dst && dst->memcpy_path != 0, src->r, src->cap, src_idx_dev, dst->r, dst->cap, dst_idx_dev, count, false);
}

int ngw_snapshot_expand(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, ngw_snapshot* dst,
                        const int32_t* dst_slots_dev, int64_t count, int32_t* reward_dev, uint8_t* done_dev, uint32_t* info_dev) {
    if (!h || !dst || !actions_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    Source from;
    if (int rc = step_pairs_args(h, src, src_idx_dev, dst, dst_slots_dev, count, "expand", "ngw_snapshot_expand", &from)) return rc;
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    const NgwLaunch a = step_block(h);
    NgwExpand x{};
    x.src = from.r; x.dst = dst->r;
    x.si = src_idx_dev; x.di = dst_slots_dev; x.actions = actions_dev;
    x.reward = reward_dev; x.done = done_dev; x.info = info_dev;
    x.count = (int32_t)count; x.src_rows = (int32_t)from.rows; x.dst_rows = (int32_t)dst->cap;
    HIP_TRY(ngw_expand_launch(h->dspec, &a, &x, h->ext, h->lds_bytes, h->stream));
    return NGW_OK;
}

int ngw_snapshot_rollout(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                         ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev,
                         uint32_t* info_dev) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = PLAIN; p.plan.actions = actions_dev; p.plan.stride = pair_stride;
    return step_pairs(h, p);
}

int ngw_snapshot_rollout_path(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                              const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev,
                              uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = PATH; p.plan.actions = actions_dev; p.plan.stride = pair_stride;
    p.pa.limits = limits_dev; p.pa.fields = fields; p.pa.keys = keys_dev; p.pa.keys_stride = keys_stride;
    return step_pairs(h, p);
}

int ngw_snapshot_playout_weighted(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed,
                                  uint64_t first_pair, const float* weights_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                                  int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev,
                                  int64_t actions_stride) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = PLAIN; p.draws = true; p.draw.seed = seed; p.draw.first_pair = first_pair; p.draw.weights = weights_dev;
    p.draw.first_action = first_action_dev; p.draw.actions = actions_dev; p.draw.stride = actions_stride;
    return step_pairs(h, p);
}

int ngw_snapshot_playout_path(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                              const float* weights_dev, const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                              int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride,
                              uint32_t fields, uint64_t* keys_dev, int64_t keys_stride) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = PATH; p.draws = true; p.draw.seed = seed; p.draw.first_pair = first_pair; p.draw.weights = weights_dev;
    p.draw.first_action = first_action_dev; p.draw.actions = actions_dev; p.draw.stride = actions_stride;
    p.pa.limits = limits_dev; p.pa.fields = fields; p.pa.keys = keys_dev; p.pa.keys_stride = keys_stride;
    return step_pairs(h, p);
}

int ngw_snapshot_rollout_traj(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                              const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev,
                              uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev,
                              int64_t rewards_stride, void* obs_dev, int64_t obs_stride) {
    return ngw_snapshot_rollout_traj_views(h, src, src_idx_dev, actions_dev, pair_stride, n_steps, limits_dev, dst, dst_slots_dev, count, ret_dev, length_dev, ended_dev,
                                           info_dev, fields, keys_dev, keys_stride, rewards_dev, rewards_stride, obs_dev, obs_stride, nullptr);
}

int ngw_snapshot_rollout_traj_views(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, const int32_t* actions_dev, int64_t pair_stride, int32_t n_steps,
                                    const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int64_t count, int32_t* ret_dev, int32_t* length_dev,
                                    uint8_t* ended_dev, uint32_t* info_dev, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev,
                                    int64_t rewards_stride, void* obs_dev, int64_t obs_stride, const ngw_traj_views* views) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = TRAJ; p.plan.actions = actions_dev; p.plan.stride = pair_stride;
    p.pa.limits = limits_dev; p.pa.fields = fields; p.pa.keys = keys_dev; p.pa.keys_stride = keys_stride;
    p.ta.rewards = rewards_dev; p.ta.rewards_stride = rewards_stride; p.ta.obs = obs_dev; p.ta.obs_stride = obs_stride;
    views_arg(p.ta, views);
    return step_pairs(h, p);
}

int ngw_snapshot_playout_traj(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                              const float* weights_dev, const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                              int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride,
                              uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride, uint64_t* masks_dev,
                              int64_t masks_stride, void* obs_dev, int64_t obs_stride) {
    return ngw_snapshot_playout_traj_views(h, src, src_idx_dev, count, n_steps, seed, first_pair, weights_dev, limits_dev, dst, dst_slots_dev, ret_dev, length_dev,
                                           ended_dev, info_dev, first_action_dev, actions_dev, actions_stride, fields, keys_dev, keys_stride, rewards_dev, rewards_stride,
                                           masks_dev, masks_stride, obs_dev, obs_stride, nullptr);
}

int ngw_snapshot_playout_traj_views(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                                    const float* weights_dev, const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                                    int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev,
                                    int64_t actions_stride, uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride,
                                    uint64_t* masks_dev, int64_t masks_stride, void* obs_dev, int64_t obs_stride, const ngw_traj_views* views) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = TRAJ; p.draws = true; p.draw.seed = seed; p.draw.first_pair = first_pair; p.draw.weights = weights_dev;
    p.draw.first_action = first_action_dev; p.draw.actions = actions_dev; p.draw.stride = actions_stride;
    p.pa.limits = limits_dev; p.pa.fields = fields; p.pa.keys = keys_dev; p.pa.keys_stride = keys_stride;
    p.ta.rewards = rewards_dev; p.ta.rewards_stride = rewards_stride; p.ta.obs = obs_dev; p.ta.obs_stride = obs_stride; p.ta.masks = masks_dev; p.ta.masks_stride = masks_stride;
    views_arg(p.ta, views);
    return step_pairs(h, p);
}

int ngw_snapshot_playout_guided(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                                const float* weights_dev, const int32_t* limits_dev, ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev,
                                int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev, int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride,
                                uint32_t fields, uint64_t* keys_dev, int64_t keys_stride, int32_t* rewards_dev, int64_t rewards_stride, uint64_t* masks_dev,
                                int64_t masks_stride, void* obs_dev, int64_t obs_stride, const ngw_traj_views* views, ngw_key_table* table,
                                const float* table_weights_dev, int32_t* where_dev, int64_t where_stride, int32_t* depth_dev, int32_t outside) {
    Pairs p{};
    p.src = src; p.src_idx = src_idx_dev; p.dst = dst; p.dst_slots = dst_slots_dev; p.count = count; p.n_steps = n_steps;
    p.ret = ret_dev; p.length = length_dev; p.ended = ended_dev; p.info = info_dev;
    p.form = TRAJ; p.draws = true; p.draw.seed = seed; p.draw.first_pair = first_pair; p.draw.weights = weights_dev;
    p.draw.first_action = first_action_dev; p.draw.actions = actions_dev; p.draw.stride = actions_stride;
    p.pa.limits = limits_dev; p.pa.fields = fields; p.pa.keys = keys_dev; p.pa.keys_stride = keys_stride;
    p.ta.rewards = rewards_dev; p.ta.rewards_stride = rewards_stride; p.ta.obs = obs_dev; p.ta.obs_stride = obs_stride; p.ta.masks = masks_dev; p.ta.masks_stride = masks_stride;
    views_arg(p.ta, views);
    p.guided = true;
    p.ga.table = table; p.ga.rows = table_weights_dev; p.ga.where = where_dev; p.ga.where_stride = where_stride; p.ga.depth = depth_dev; p.ga.outside = outside;
    return step_pairs(h, p);
}

int ngw_snapshot_playout(ngw_handle* h, ngw_snapshot* src, const int32_t* src_idx_dev, int64_t count, int32_t n_steps, uint64_t seed, uint64_t first_pair,
                         ngw_snapshot* dst, const int32_t* dst_slots_dev, int32_t* ret_dev, int32_t* length_dev, uint8_t* ended_dev, uint32_t* info_dev,
                         int32_t* first_action_dev, int32_t* actions_dev, int64_t actions_stride) {
    return ngw_snapshot_playout_weighted(h, src, src_idx_dev, count, n_steps, seed, first_pair, nullptr, dst, dst_slots_dev, ret_dev, length_dev, ended_dev, info_dev,
                                         first_action_dev, actions_dev, actions_stride);
}

int ngw_snapshot_lidar(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, void* rows_dev) {
    if (int rc = slot_obs_args(h, s, rows_dev, slots_dev, count, "lidar observation")) return rc;
    if (!h->lidar_len) return fail(NGW_E_INVALID_ARG, "ngw_snapshot_lidar before ngw_lidar_configure");
    if (!h->lidar_lds) return fail(NGW_E_INVALID_ARG, "map_size %d: the lidar observation keeps a wavefront's 64 maps in LDS (> 160 KiB)", h->proto.S);
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    NgwLaunch a = h->lidar_proto;                     // the stand-alone launch's LDS layout and the current row format, whichever form the env's fused path uses
    a.b = h->b;
    a.lout = static_cast<int32_t*>(rows_dev);
    NgwSlotObs x = slot_obs(h, s, slots_dev, count);
    HIP_TRY(ngw_slot_lidar_launch(&a, &x, h->lidar_lds, h->stream));
    return NGW_OK;
}

int ngw_snapshot_agent_view(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, int view_size, int8_t* view_dev, int32_t* facing_dev,
                            int32_t* inv_dev) {
    const void* any = view_dev ? (const void*)view_dev : (facing_dev ? (const void*)facing_dev : (const void*)inv_dev);
    if (int rc = slot_obs_args(h, s, any, slots_dev, count, "agent view")) return rc;
    if (view_size < 1 || view_size > 127) return fail(NGW_E_INVALID_ARG, "view_size must be in 1..127");
    const size_t W = 2 * (size_t)view_size + 1, bytes = (size_t)count * W * W;
    if (bytes + 4 > 0xffffffffull) return fail(NGW_E_INVALID_ARG, "agent view of %zu B exceeds the 4 GiB index range", bytes);
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    NgwSlotObs x = slot_obs(h, s, slots_dev, count);
    x.view = reinterpret_cast<uint32_t*>(view_dev); x.facing = facing_dev; x.inv = inv_dev;
    x.n_dwords = (uint32_t)((bytes + 3) / 4); x.S = h->proto.S; x.K = h->proto.K; x.V = view_size;
    HIP_TRY(ngw_slot_view_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_snapshot_action_mask(ngw_handle* h, ngw_snapshot* s, const int32_t* slots_dev, int64_t count, uint64_t* masks_dev) {
    if (int rc = slot_obs_args(h, s, masks_dev, slots_dev, count, "action masks")) return rc;
    if (int rc = enter(h)) return rc;
    if (count == 0) return NGW_OK;
    NgwSlotObs x = slot_obs(h, s, slots_dev, count);
    HIP_TRY(ngw_slot_mask_launch(h->dspec, &x, h->proto.S, h->proto.K, h->ext, masks_dev, h->stream));
    return NGW_OK;
}

int ngw_sample_actions(ngw_handle* h, ngw_snapshot* src, const int32_t* idx_dev, int64_t count, const float* weights_dev, int64_t weight_stride,
                       uint64_t seed, uint64_t first_pair, uint32_t t, int32_t* actions_dev, float* mass_dev, uint64_t* masks_dev) {
    if (!h || !weights_dev || !actions_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (src && !is_open(h->snaps, src)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    const Source from = source_of(h, src);
    if (count < 0 || count > 0x7FFFFFFFll || weight_stride < count)
        return fail(NGW_E_INVALID_ARG, "sampled actions of %lld states with a weight stride of %lld", (long long)count, (long long)weight_stride);
    if (!idx_dev && count > from.rows) return fail(NGW_E_INVALID_ARG, "sampled actions of %lld states from %lld %s", (long long)count, (long long)from.rows, from.unit);
    if (int rc = enter(h)) return rc;                 // (src == NULL: the one-env loop has ended, HBM holds the env's state)
    if (count == 0) return NGW_OK;
    NgwSample x{};
    x.src = from.r; x.idx = idx_dev; x.flags = h->b.flags;
    x.weights = weights_dev; x.stride = weight_stride; x.seed = seed; x.first_pair = first_pair; x.t = t;
    x.actions = actions_dev; x.mass = mass_dev; x.masks = masks_dev;
    x.count = (int32_t)count; x.rows = (int32_t)from.rows;
    HIP_TRY(ngw_sample_launch(h->dspec, &x, h->proto.S, h->proto.K, h->ext, h->stream));
    return NGW_OK;
}

int ngw_state_keys(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, uint32_t fields, uint64_t* keys_dev) {
    if (!h || !keys_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (s && !is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (int rc = key_args(fields)) return rc;
    const Source from = source_of(h, s);
    if (count < 0 || count > 0x7FFFFFFFll * NGW_EPB) return fail(NGW_E_INVALID_ARG, "state keys of %lld rows", (long long)count);
    if (!idx_dev && count > from.rows) return fail(NGW_E_INVALID_ARG, "state keys of %lld rows from %lld %s", (long long)count, (long long)from.rows, from.unit);
    if (int rc = enter(h)) return rc;                 // (s == NULL: the one-env loop has ended, HBM holds the env's state - what ngw_snapshot_expand relies on)
    if (count == 0) return NGW_OK;
    NgwKeys x{};
    x.src = from.r; x.idx = idx_dev; x.flags = h->b.flags; x.keys = keys_dev;
    x.count = count; x.rows = (int32_t)from.rows; x.S2 = h->proto.S2; x.K = h->proto.K; x.fields = fields;
    HIP_TRY(ngw_keys_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_successor_keys(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, uint32_t fields, uint64_t* keys_dev, int32_t* reward_dev,
                       uint8_t* done_dev, uint32_t* info_dev) {
    if (!h || !keys_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (s && !is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (int rc = key_args(fields)) return rc;
    const Source from = source_of(h, s);
    const int64_t A = h->spec.n_actions;
    // (the flattened [count * A] keys are what ngw_state_keys and the key table take: the same range)
    if (count < 0 || count > 0x7FFFFFFFll * NGW_EPB / A) return fail(NGW_E_INVALID_ARG, "successor keys of %lld rows by %lld actions", (long long)count, (long long)A);
    if (!idx_dev && count > from.rows) return fail(NGW_E_INVALID_ARG, "successor keys of %lld rows from %lld %s", (long long)count, (long long)from.rows, from.unit);
    const size_t lds = NGW_SUCC_LDS_BYTES(h->proto.MS, h->proto.KP);
    if (lds > NGW_SUCC_LDS_MAX)
        return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps two sets of a wavefront's 64 maps in LDS (ngw_successor_keys: the stepped rows and "
                                       "the parents they are compared with) and they need %zu B, more than 160 KiB; ngw_snapshot_expand followed by "
                                       "ngw_state_keys is available", h->proto.S, lds);
    if (int rc = enter(h)) return rc;                 // (s == NULL: the one-env loop has ended, HBM holds the env's state)
    if (count == 0) return NGW_OK;
    const NgwLaunch a = step_block(h);
    NgwSuccessors x{};
    x.src = from.r; x.idx = idx_dev; x.keys = keys_dev;
    x.reward = reward_dev; x.done = done_dev; x.info = info_dev;
    x.count = count; x.rows = (int32_t)from.rows; x.fields = fields;
    HIP_TRY(ngw_successors_launch(h->dspec, &a, &x, h->ext, h->stream));
    return NGW_OK;
}

int ngw_snapshot_walk(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, const int32_t* items_dev, int32_t n_steps, int32_t* dist_dev,
                      int32_t* plans_dev, int32_t* length_dev) {
    if (!h) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (s && !is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (!items_dev && (plans_dev || length_dev)) return fail(NGW_E_INVALID_ARG, "walk plans without items: one item id per row expected");
    if (!dist_dev && !plans_dev && !length_dev) return fail(NGW_E_INVALID_ARG, "walk without an output: nothing to do");
    if (items_dev && n_steps < 1) return fail(NGW_E_INVALID_ARG, "walk plans of %d steps", (int)n_steps);
    const Source from = source_of(h, s);
    if (count < 0 || count > 0x7FFFFFFFll) return fail(NGW_E_INVALID_ARG, "walk of %lld rows", (long long)count);
    if (!idx_dev && count > from.rows) return fail(NGW_E_INVALID_ARG, "walk of %lld rows from %lld %s", (long long)count, (long long)from.rows, from.unit);
    // the ids a plan is written in: the lowest action id of each of the three kinds (a remapped action table keeps its kinds)
    int32_t act[3] = {-1, -1, -1};
    for (int a = h->spec.n_actions - 1; a >= 0; a--)
        if (h->spec.act_kind[a] <= NGW_ACT_RIGHT) act[h->spec.act_kind[a]] = a;
    if (plans_dev && (act[NGW_ACT_FORWARD] < 0 || act[NGW_ACT_LEFT] < 0 || act[NGW_ACT_RIGHT] < 0))
        return fail(NGW_E_INVALID_ARG, "walk plans need a Forward, a Left and a Right action; this spec has no %s (the distances are available)",
                    act[NGW_ACT_FORWARD] < 0 ? "Forward" : (act[NGW_ACT_LEFT] < 0 ? "Left" : "Right"));
    if (int rc = enter(h)) return rc;                 // (s == NULL: the one-env loop has ended, HBM holds the env's state)
    if (count == 0) return NGW_OK;
    NgwWalk x{};
    x.src = from.r; x.idx = idx_dev; x.items = items_dev; x.flags = h->b.flags;
    x.dist = dist_dev; x.plans = plans_dev; x.length = length_dev;
    x.count = count; x.rows = (int32_t)from.rows; x.S = h->proto.S; x.K = h->proto.K; x.T = items_dev ? n_steps : 0; x.SP = NGW_WALK_SP(h->proto.S);
    x.act_forward = act[NGW_ACT_FORWARD]; x.act_left = act[NGW_ACT_LEFT]; x.act_right = act[NGW_ACT_RIGHT];
    HIP_TRY(ngw_walk_launch(&x, h->stream));
    return NGW_OK;
}

int ngw_snapshot_get(ngw_handle* h, ngw_snapshot* s, int64_t first, int64_t count, int8_t* map, int32_t* loc, int32_t* facing, int32_t* inv,
                     int32_t* selected, int32_t* step_count, uint32_t* episode) {
    if (!h || !s) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (!is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    if (first < 0 || count < 0 || first + count > s->cap) return fail(NGW_E_INVALID_ARG, "slot range [%lld, +%lld) out of bounds", (long long)first, (long long)count);
    if (int rc = enter(h)) return rc;
    const size_t n = (size_t)count, f = (size_t)first, S2 = (size_t)h->proto.S2, K = (size_t)h->proto.K;
    D2H(map, s->r.map + f * S2, n * S2);
    D2H(loc, s->r.loc + f * 2, n * 2 * sizeof(int32_t));
    D2H(facing, s->r.facing + f, n * sizeof(int32_t));
    D2H(inv, s->r.inv + f * K, n * K * sizeof(int32_t));
    D2H(step_count, s->r.step_count + f, n * sizeof(int32_t));
    D2H(episode, s->r.episode + f, n * sizeof(uint32_t));
    std::vector<uint8_t> sel;
    if (selected) {
        sel.resize(n);
        HIP_TRY(hipMemcpyAsync(sel.data(), s->r.selected + f, n, hipMemcpyDefault, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (selected)
        for (size_t i = 0; i < n; i++) selected[i] = sel[i];
    return NGW_OK;
}

}  // extern "C"
