// fake_kernels.cpp - one stub per *_launch that gym_novel_gridworlds_amd/csrc/ngw_device.h declares (a launcher without one fails the link).
// A stub runs no algorithm and says nothing about what a kernel computes.  It touches memory over the extent the kernel is ALLOWED to use, as
// ngw_device.h and include/ngw.h document it for each struct member, so that AddressSanitizer checks the host's sizing against it:
//   in(p, n)     an input array: read from its first to its last element
//   out(p, n, v) an output array: written from its first to its last element with a recognisable value
//   inout(p, n)  an array the kernel reads and updates: read whole, first and last element written back unchanged (its content stays)
// The extents are restated here from the documentation, never taken from the .cpp that computes the allocation.  Values the host acts on are
// sane: sequence words get the sequence asked for, counters and error flags 0, index lists NGW_IDX_NONE, counts 0.
// Full extents: search, roots, recipe, the six tree launches, select, frontier, alloc, the table launches, snapshot, expand, keys, successors, walk,
// the step / reset / pack / diff / wire launches.  Partial (output arrays only, inputs and the LDS layout not checked): lidar, boards, agent view, masks, lookahead, plans,
// slot observers, sample, and the seven rollout / playout launchers, of which only the [count] report arrays are written - their [step][stride]
// outputs (actions, keys, rewards, masks, obs, views, where) are NOT touched (the tree stubs read the ones a tree-search run records).  ngw_solo_launch touches nothing: the one-env loop is out of scope
// and the harness runs with NGW_SOLO=0.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gym_novel_gridworlds_amd/csrc/ngw_device.h"

namespace {

volatile uint64_t g_sink;

// HOSTCHECK_STUB_COUNTS=1: how often each stub (and each form of the step launch) ran, printed at exit - the test's proof that a scenario
// reached the paths it is about
struct Hits {
    static const int MAX = 96;
    const char* name[MAX]; long long n[MAX]; int used = 0;
    void hit(const char* s) {
        for (int i = 0; i < used; i++) if (!strcmp(name[i], s)) { n[i]++; return; }
        if (used < MAX) { name[used] = s; n[used++] = 1; }
    }
    ~Hits() {
        if (!getenv("HOSTCHECK_STUB_COUNTS")) return;
        for (int i = 0; i < used; i++) fprintf(stderr, "stub %s %lld\n", name[i], n[i]);
    }
} g_hits;
#define HIT(s) g_hits.hit(s)

// Inside ONE allocation the sanitizer sees no border between two arrays: a carve-up that puts one array a word early overlaps its neighbour and
// no redzone is crossed.  So every stub also notes each range it touches, and when it returns no range that is written may overlap another one,
// unless the two are the same range and at most one of them is written (a call may alias on purpose: source and destination rows of one snapshot).
// Two WRITTEN members with the same bounds are a dropped offset in a carve-up (f = h, tags = values) and end the program too; so a stub touches
// each member once.
struct Range { const char* lo; const char* hi; bool written; };
struct Scope {
    static const int MAX = 128;
    Range r[MAX]; int used = 0; const char* stub;
    static Scope* cur;
    Scope* outer;
    explicit Scope(const char* name) : stub(name), outer(cur) { cur = this; }
    void note(const void* p, size_t bytes, bool written) {
        if (!p || !bytes) return;
        if (used == MAX) { fprintf(stderr, "hostcheck: %s: more than %d ranges in one launch: raise Scope::MAX\n", stub, MAX); abort(); }
        r[used++] = Range{static_cast<const char*>(p), static_cast<const char*>(p) + bytes, written};
    }
    ~Scope() {
        cur = outer;
        for (int i = 0; i < used; i++)
            for (int j = i + 1; j < used; j++) {
                if (!(r[i].written || r[j].written) || r[i].hi <= r[j].lo || r[j].hi <= r[i].lo) continue;
                if (r[i].lo == r[j].lo && r[i].hi == r[j].hi && !(r[i].written && r[j].written)) continue;
                fprintf(stderr, "hostcheck: %s: two arrays of one launch overlap: [%p, +%zu) and [%p, +%zu) share %zu bytes\n", stub, (const void*)r[i].lo,
                        (size_t)(r[i].hi - r[i].lo), (const void*)r[j].lo, (size_t)(r[j].hi - r[j].lo),
                        (size_t)((r[i].hi < r[j].hi ? r[i].hi : r[j].hi) - (r[i].lo > r[j].lo ? r[i].lo : r[j].lo)));
                abort();
            }
    }
};
Scope* Scope::cur = nullptr;
void note(const void* p, size_t bytes, bool written) { if (Scope::cur) Scope::cur->note(p, bytes, written); }

void in_bytes(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    unsigned char tmp[4096];
    const unsigned char* s = static_cast<const unsigned char*>(p);
    uint64_t acc = 0;
    while (bytes) {
        const size_t k = bytes < sizeof(tmp) ? bytes : sizeof(tmp);
        memcpy(tmp, s, k);                             // (checked by the sanitizer's memcpy over the whole range)
        acc += tmp[0] + tmp[k - 1];
        s += k; bytes -= k;
    }
    g_sink = g_sink + acc;
}
template <typename T> void in(const T* p, size_t n) { note(p, n * sizeof(T), false); in_bytes(p, n * sizeof(T)); }
template <typename T> void out(T* p, size_t n, T v) {
    if (!p) return;
    note(p, n * sizeof(T), true);
    for (size_t i = 0; i < n; i++) p[i] = v;
}
template <typename T> void inout(T* p, size_t n) {
    if (!p || !n) return;
    in_bytes(p, n * sizeof(T));
    note(p, n * sizeof(T), true);
    volatile T* q = p;
    q[0] = q[0];
    q[n - 1] = q[n - 1];
}
void out_bytes(void* p, size_t bytes, int v) { note(p, bytes, true); if (p && bytes) memset(p, v, bytes); }
void flag_word(uint32_t* f) { inout(f, 1); }           // an error-flags word: raised with an atomic OR; the stub raises nothing

size_t pad64(int64_t n) { return (size_t)((n + NGW_EPB - 1) / NGW_EPB * NGW_EPB); }
size_t ceil_div(int64_t a, int64_t b) { return (size_t)((a + b - 1) / b); }

// NgwSnapRows: [rows][S*S] map, [rows][2] loc, [rows] facing, [rows][K] inv, [rows] selected / step_count / episode
void rows_in(const NgwSnapRows& r, size_t rows, size_t S2, size_t K) {
    in(r.map, rows * S2); in(r.loc, rows * 2); in(r.facing, rows); in(r.inv, rows * K); in(r.selected, rows); in(r.step_count, rows); in(r.episode, rows);
}
void rows_inout(const NgwSnapRows& r, size_t rows, size_t S2, size_t K, bool episode = true) {
    inout(r.map, rows * S2); inout(r.loc, rows * 2); inout(r.facing, rows); inout(r.inv, rows * K); inout(r.selected, rows); inout(r.step_count, rows);
    if (episode) inout(r.episode, rows);
}

// NgwBufs: every array [n_pad] rows; perm [S*S][n_pad] uint16; brd [n_pad][BS]; flags [1]; flags_host: word 0 and word NGW_SEQ_WORD
void bufs_inout(const NgwBufs& b, size_t np, size_t S2, size_t K, size_t BS, bool outs) {
    inout(b.map, np * S2); inout(b.loc, np * 2); inout(b.facing, np); inout(b.inv, np * K); inout(b.selected, np); inout(b.step_count, np);
    inout(b.episode, np);
    if (outs) { out(b.reward, np, (int32_t)0); out(b.done, np, (uint8_t)0); out(b.info, np, (uint32_t)0); }
    flag_word(b.flags);
    inout(b.perm, S2 * np);
    inout(b.brd, np * BS);
}
// NgwNx: [depth][n_pad] rows of every array, depth = dmask + 1, n_pad = stride; slow [2], slow_host [2]
void nx_inout(const NgwNx& x, size_t S2, size_t K, size_t BS) {
    if (!x.episode) return;
    const size_t rows = (size_t)(x.dmask + 1) * (size_t)x.stride;
    inout(x.map, rows * S2); inout(x.loc, rows * 2); inout(x.facing, rows); inout(x.inv, rows * K); inout(x.episode, rows); inout(x.brd, rows * BS);
    inout(x.slow, 2); inout(x.slow_host, 2);
}
// the host mirror of a single-wavefront handle (NgwMirror: "the same rows"), then the sequence word
void mirror_out(const NgwDevSpec* d, const NgwBufs& b, size_t np, size_t S2, size_t K, uint32_t seq) {
    if (!seq || !b.flags_host) return;
    HIT("mirror_out");
    const NgwMirror& m = d->mir;
    if (m.map) {
        inout(m.map, np * S2); inout(m.loc, np * 2); inout(m.facing, np); inout(m.inv, np * K); inout(m.selected, np); inout(m.step_count, np);
        out(m.reward, np, (int32_t)0); out(m.done, np, (uint8_t)0); out(m.info, np, (uint32_t)0);
    }
    b.flags_host[0] = 0;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    b.flags_host[NGW_SEQ_WORD] = seq;                  // what ngwh::wait_seq polls
}
// the lidar rows of a launch block: [rows] rows of l_rb bytes
void lidar_rows_out(const NgwLaunch* a, void* rows_ptr, size_t rows) { out_bytes(rows_ptr, rows * (size_t)a->l_rb, 0x5A); }

// what the seven kernels that step saved rows share: the parents, the lists, the [count] reports, the kept end states
template <class X>
void pairs_partial(const NgwDevSpec* d, const NgwLaunch* a, const X* x) {
    in(d, 1);
    const size_t S2 = (size_t)a->S2, K = (size_t)a->K, n = (size_t)x->count;
    rows_in(x->src, (size_t)x->src_rows, S2, K);
    in(x->si, n);
    if (x->keep) { in(x->di, n); rows_inout(x->dst, (size_t)x->dst_rows, S2, K); }
    out(x->ret, n, (int32_t)0); out(x->length, n, (int32_t)0); out(x->ended, n, (uint8_t)0); out(x->info, n, (uint32_t)0);
    flag_word(a->b.flags);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- steps, resets, refills, rollouts of the handle's own state
hipError_t ngw_launch(const NgwDevSpec* dspec, const NgwLaunch* a, int, int feat, unsigned grid, size_t, hipStream_t) { HIT("ngw_launch"); Scope scope_("ngw_launch");
    in(dspec, 1);
    // a slice (bid0, launch_step_slice) brings pointers shifted to its first env and n = its env count: whole wavefronts of it
    const size_t np = a->bid0 || (int64_t)grid * NGW_EPB < a->n_pad ? (size_t)grid * NGW_EPB : (size_t)a->n_pad;
    const size_t n = (size_t)a->n, S2 = (size_t)a->S2, K = (size_t)a->K, BS = (size_t)a->BS;
    if (a->mode >= NGW_MODE_DBG_NOP) return hipSuccess;
    if (a->mode == NGW_MODE_REFILL) {
        HIT("ngw_launch:refill");
        // a.b = one slot of the shadow set (map, loc, facing, inv, episode, brd; flags, perm the handle's), a.actions = the main episode[]
        inout(a->b.map, np * S2); inout(a->b.loc, np * 2); inout(a->b.facing, np); inout(a->b.inv, np * K); inout(a->b.episode, np);
        inout(a->b.brd, np * BS); inout(a->b.perm, S2 * np); flag_word(a->b.flags);
        in(reinterpret_cast<const uint32_t*>(a->actions), np);
        inout(dspec->nx.slow, 2); inout(dspec->nx.slow_host, 2);
        return hipSuccess;
    }
    bufs_inout(a->b, np, S2, K, BS, true);
    if (a->mode == NGW_MODE_STEP) {
        if (a->use_action0 == 2) in(reinterpret_cast<const uint8_t*>(a->actions), n);      // one BYTE per env
        else if (a->use_action0 == 1) in(a->actions, 1);                                      // "still points at valid device memory"
        else in(a->actions, n);
    }
    if (a->mode == NGW_MODE_ROLLOUT_ACT) in(a->actions, (size_t)(a->n_steps - 1) * (size_t)a->t0 + n);
    if (a->mode == NGW_MODE_RESET) in(a->reset_mask, n);
    if (a->mode == NGW_MODE_ROLLOUT || a->mode == NGW_MODE_ROLLOUT_ACT) {
        if (a->row_reward) out(a->row_reward, (size_t)(a->n_steps - 1) * (size_t)a->row_stride + n, (int32_t)0);
        if (a->row_done) out(a->row_done, (size_t)(a->n_steps - 1) * (size_t)a->row_stride + n, (uint8_t)0);
        inout(a->acc, 4 * np);
    }
    // the cold path: prepared next episodes consumed, terminal observations captured
    nx_inout(dspec->nx, S2, K, dspec->nx.brd ? BS : 0);
    if (dspec->term.map) { inout(dspec->term.map, np * S2); inout(dspec->term.loc, np * 2); inout(dspec->term.facing, np); inout(dspec->term.inv, np * K); }
    if (feat & NGW_FEAT_LIDAR) { HIT("ngw_launch:lidar"); in(a->lcfg, 1); lidar_rows_out(a, a->lout, np); }
    if (feat & NGW_FEAT_MASK) out(dspec->amask, np, (uint64_t)0);
    if (feat & NGW_FEAT_VIEW) { const NgwLaunchView* v = static_cast<const NgwLaunchView*>(a); out(v->view, (size_t)v->n_dwords, 0x5A5A5A5Au); }
    if (feat & NGW_FEAT_WIRE) {
        HIT("ngw_launch:wire");
        const NgwWT& w = dspec->wt;                    // [n] rows of the caller's block, flags [2], the device counter, [n_pad] lidar rows
        inout(w.map, n * S2); inout(w.inv, n * K); out(w.pose, n, 0x01010101u); out(w.reward, n, (int32_t)0); out(w.done, n, (uint8_t)0); out(w.info, n, 0u);
        inout(w.count, 1);
        if (w.rows) lidar_rows_out(a, w.rows, np);
        w.flags[0] = 0;
        __atomic_thread_fence(__ATOMIC_RELEASE);
        w.flags[1] = a->seq;                           // the sequence number ngw_step_host_packed polls
    } else
        mirror_out(dspec, a->b, np, S2, K, a->seq);
    return hipSuccess;
}

hipError_t ngw_reset_fast_launch(const NgwDevSpec* dspec, const struct NgwResetFast* a, int, int subset, unsigned grid, size_t, hipStream_t) { HIT("ngw_reset_fast_launch"); Scope scope_("ngw_reset_fast_launch");
    in(dspec, 1);
    const size_t np = (size_t)grid * NGW_EPB, n = (size_t)a->n, S2 = (size_t)a->S2, K = (size_t)a->K, BS = a->boards ? (size_t)a->BS : 0;
    if (a->mode == NGW_MODE_RESET) {
        bufs_inout(a->main, np, S2, K, BS, false);      // (the episode counters and the flags word among them: a->flags is main.flags)
        if (a->flags != a->main.flags) flag_word(a->flags);
        in(a->reset_mask, n);
    } else {
        inout(a->main.episode, np);
        flag_word(a->flags);
    }
    nx_inout(a->nx, S2, K, a->nx.brd ? BS : 0);
    if (subset) in(a->pctq, 64);
    if (a->mode == NGW_MODE_RESET) mirror_out(dspec, a->main, np, S2, K, a->seq);
    return hipSuccess;
}

// ---------------------------------------------------------------- pack / diff / wire
hipError_t ngw_pack_launch(const struct NgwPack* p, hipStream_t) { HIT("ngw_pack_launch"); Scope scope_("ngw_pack_launch");
    for (int r = 0; r < p->n_regions; r++) { note(p->src[r], (size_t)p->nbytes[r], false); in_bytes(p->src[r], (size_t)p->nbytes[r]); out_bytes(p->dst[r], (size_t)p->nbytes[r], 0); }
    return hipSuccess;
}
static void diff_touch(const struct NgwDiff* p) {
    for (int r = 0; r < p->n_regions; r++) {
        note(p->cur[r], (size_t)p->nbytes[r], false); in_bytes(p->cur[r], (size_t)p->nbytes[r]);
        inout(p->shadow[r], (size_t)p->nbytes[r]);
        inout(p->host[r], (size_t)p->nbytes[r]);
    }
}
static void wire_touch(const struct NgwWire* w) {
    const size_t n = (size_t)w->n;
    in(w->loc, 2 * n); in(w->facing, n); in(w->selected, n); in(w->reward, n); in(w->done, n); in(w->info, n); in(w->flags, 1);
    out(w->pose, n, 0x01010101u); out(w->reward32, n, (int32_t)0); out(w->done8, n, (uint8_t)0); out(w->info32, n, 0u); out(w->flags_out, 1, 0u);
}
hipError_t ngw_diff_launch(const struct NgwDiff* p, hipStream_t) { HIT("ngw_diff_launch"); Scope scope_("ngw_diff_launch"); diff_touch(p); return hipSuccess; }
hipError_t ngw_wire_launch(const struct NgwWire* p, hipStream_t) { HIT("ngw_wire_launch"); Scope scope_("ngw_wire_launch"); wire_touch(p); return hipSuccess; }
hipError_t ngw_diff_wire_launch(const struct NgwDiff* p, const struct NgwWire* w, hipStream_t) { HIT("ngw_diff_wire_launch"); Scope scope_("ngw_diff_wire_launch"); diff_touch(p); wire_touch(w); return hipSuccess; }

// ---------------------------------------------------------------- partial: observation wrappers, masks, lookahead, plans (outputs only)
hipError_t ngw_agent_view_launch(const int8_t*, const int32_t*, uint32_t* o, uint32_t n_dwords, int, int, hipStream_t) { HIT("ngw_agent_view_launch"); Scope scope_("ngw_agent_view_launch");
    out(o, (size_t)n_dwords, 0x5A5A5A5Au);
    return hipSuccess;
}
hipError_t ngw_lidar_launch(const NgwLaunch* a, int, unsigned grid, size_t, hipStream_t) { HIT("ngw_lidar_launch"); Scope scope_("ngw_lidar_launch");
    in(a->lcfg, 1);
    lidar_rows_out(a, a->lout, (size_t)grid * NGW_EPB);
    return hipSuccess;
}
hipError_t ngw_boards_launch(const NgwLaunch* a, int, const int8_t* map, uint32_t* brd, int64_t rows, size_t, hipStream_t) { HIT("ngw_boards_launch"); Scope scope_("ngw_boards_launch");
    in(map, (size_t)rows * (size_t)a->S2);
    out(brd, (size_t)rows * (size_t)a->BS, 0u);
    return hipSuccess;
}
hipError_t ngw_lidar_boards_launch(const NgwLaunch* a, unsigned grid, size_t, hipStream_t) { HIT("ngw_lidar_boards_launch"); Scope scope_("ngw_lidar_boards_launch");
    lidar_rows_out(a, a->lout, (size_t)grid * NGW_EPB);
    return hipSuccess;
}
hipError_t ngw_solo_launch(const NgwDevSpec*, const struct NgwSolo*, int, size_t, hipStream_t) { HIT("ngw_solo_launch"); Scope scope_("ngw_solo_launch"); return hipSuccess; }   // out of scope: touches nothing
hipError_t ngw_mask_launch(const NgwDevSpec*, const NgwBufs*, int64_t, int, int, int, uint64_t* o, unsigned grid, hipStream_t) { HIT("ngw_mask_launch"); Scope scope_("ngw_mask_launch");
    out(o, (size_t)grid * NGW_EPB, (uint64_t)0);       // [n_pad] words
    return hipSuccess;
}
hipError_t ngw_lookahead_launch(const NgwDevSpec* dspec, const NgwBufs*, int64_t, int64_t n_pad, int, int, int, int, int, int32_t* reward, uint8_t* done,
                                uint32_t* info, unsigned, hipStream_t) { HIT("ngw_lookahead_launch"); Scope scope_("ngw_lookahead_launch");
    const size_t e = (size_t)dspec->u.n_actions * (size_t)n_pad;   // action-major [n_actions][n_pad]
    out(reward, e, (int32_t)0); out(done, e, (uint8_t)0); out(info, e, 0u);
    return hipSuccess;
}
hipError_t ngw_plans_launch(const NgwDevSpec*, const NgwLaunch* a, const struct NgwPlan* pa, int, int, size_t, hipStream_t) { HIT("ngw_plans_launch"); Scope scope_("ngw_plans_launch");
    const size_t e = (size_t)pa->n_plans * (size_t)a->n_pad;       // plan-major [n_plans][n_pad]
    out(pa->ret, e, (int32_t)0); out(pa->length, e, (int32_t)0); out(pa->ended, e, (uint8_t)0); out(pa->info, e, 0u);
    return hipSuccess;
}

// ---------------------------------------------------------------- snapshots and what reads saved rows
hipError_t ngw_snapshot_launch(const struct NgwSnap* p, hipStream_t) { HIT("ngw_snapshot_launch"); Scope scope_("ngw_snapshot_launch");
    const size_t S2 = (size_t)p->S2, K = (size_t)p->K;
    rows_in(p->src, (size_t)p->src_rows, S2, K);
    rows_inout(p->dst, (size_t)p->dst_rows, S2, K, !p->keep_episode);
    in(p->si, (size_t)p->count); in(p->di, (size_t)p->count);
    flag_word(p->flags);
    return hipSuccess;
}
hipError_t ngw_expand_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwExpand* x, int, size_t, hipStream_t) { HIT("ngw_expand_launch"); Scope scope_("ngw_expand_launch");
    in(dspec, 1);
    const size_t S2 = (size_t)a->S2, K = (size_t)a->K, n = (size_t)x->count;
    rows_in(x->src, (size_t)x->src_rows, S2, K);
    rows_inout(x->dst, (size_t)x->dst_rows, S2, K);
    in(x->si, n); in(x->di, n); in(x->actions, n);
    out(x->reward, n, (int32_t)0); out(x->done, n, (uint8_t)0); out(x->info, n, 0u);
    flag_word(a->b.flags);
    return hipSuccess;
}
hipError_t ngw_slot_rollout_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwSlotRollout* x, int, size_t, hipStream_t) { HIT("ngw_slot_rollout_launch"); Scope scope_("ngw_slot_rollout_launch"); pairs_partial(d, a, x); return hipSuccess; }
hipError_t ngw_slot_rollout_path_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwSlotRollout* x, int, size_t, hipStream_t) { HIT("ngw_slot_rollout_path_launch"); Scope scope_("ngw_slot_rollout_path_launch"); pairs_partial(d, a, x); return hipSuccess; }
hipError_t ngw_slot_rollout_traj_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwSlotRollout* x, int, size_t, hipStream_t) { HIT("ngw_slot_rollout_traj_launch"); Scope scope_("ngw_slot_rollout_traj_launch"); pairs_partial(d, a, x); return hipSuccess; }
hipError_t ngw_playout_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwPlayout* x, int, size_t, hipStream_t) { HIT("ngw_playout_launch"); Scope scope_("ngw_playout_launch"); pairs_partial(d, a, x); out(x->first_action, (size_t)x->count, (int32_t)-1); return hipSuccess; }
hipError_t ngw_playout_path_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwPlayout* x, int, size_t, hipStream_t) { HIT("ngw_playout_path_launch"); Scope scope_("ngw_playout_path_launch"); pairs_partial(d, a, x); out(x->first_action, (size_t)x->count, (int32_t)-1); return hipSuccess; }
hipError_t ngw_playout_traj_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwPlayout* x, int, size_t, hipStream_t) { HIT("ngw_playout_traj_launch"); Scope scope_("ngw_playout_traj_launch"); pairs_partial(d, a, x); out(x->first_action, (size_t)x->count, (int32_t)-1); return hipSuccess; }
hipError_t ngw_playout_guided_launch(const NgwDevSpec* d, const NgwLaunch* a, const struct NgwPlayout* x, int, size_t, hipStream_t) { HIT("ngw_playout_guided_launch"); Scope scope_("ngw_playout_guided_launch");
    pairs_partial(d, a, x);
    out(x->first_action, (size_t)x->count, (int32_t)-1); out(x->depth, (size_t)x->count, (int32_t)0);
    in(x->tkey, (size_t)(x->tmask + 1));
    return hipSuccess;
}
hipError_t ngw_slot_lidar_launch(const NgwLaunch* a, const struct NgwSlotObs* x, size_t, hipStream_t) { HIT("ngw_slot_lidar_launch"); Scope scope_("ngw_slot_lidar_launch");
    in(x->slots, (size_t)x->count);
    lidar_rows_out(a, a->lout, pad64(x->count));      // [count rounded up to 64] rows of the current format
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_slot_view_launch(const struct NgwSlotObs* x, hipStream_t) { HIT("ngw_slot_view_launch"); Scope scope_("ngw_slot_view_launch");
    in(x->slots, (size_t)x->count);
    out(x->view, (size_t)x->n_dwords, 0x5A5A5A5Au); out(x->facing, (size_t)x->count, (int32_t)0); out(x->inv, (size_t)x->count * (size_t)x->K, (int32_t)0);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_slot_mask_launch(const NgwDevSpec*, const struct NgwSlotObs* x, int, int, int, uint64_t* o, hipStream_t) { HIT("ngw_slot_mask_launch"); Scope scope_("ngw_slot_mask_launch");
    in(x->slots, (size_t)x->count);
    out(o, (size_t)x->count, (uint64_t)0);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_sample_launch(const NgwDevSpec*, const struct NgwSample* x, int, int, int, hipStream_t) { HIT("ngw_sample_launch"); Scope scope_("ngw_sample_launch");
    const size_t n = (size_t)x->count;
    in(x->idx, n);
    out(x->actions, n, (int32_t)-1); out(x->mass, n, 0.0f); out(x->masks, n, (uint64_t)0);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_keys_launch(const struct NgwKeys* x, hipStream_t) { HIT("ngw_keys_launch"); Scope scope_("ngw_keys_launch");
    rows_in(x->src, (size_t)x->rows, (size_t)x->S2, (size_t)x->K);
    in(x->idx, (size_t)x->count);
    out(x->keys, (size_t)x->count, (uint64_t)0x5A5A5A5A5A5A5A5Aull);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_successors_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const struct NgwSuccessors* x, int, hipStream_t) { HIT("ngw_successors_launch"); Scope scope_("ngw_successors_launch");
    in(dspec, 1);
    const size_t n = (size_t)x->count, nA = n * (size_t)dspec->u.n_actions;    // [count * A] of every given array
    rows_in(x->src, (size_t)x->rows, (size_t)a->S2, (size_t)a->K);
    in(x->idx, n);
    out(x->keys, nA, (uint64_t)0x5A5A5A5A5A5A5A5Aull); out(x->reward, nA, (int32_t)0); out(x->done, nA, (uint8_t)0); out(x->info, nA, 0u);
    flag_word(a->b.flags);
    return hipSuccess;
}
hipError_t ngw_walk_launch(const struct NgwWalk* x, hipStream_t) { HIT("ngw_walk_launch"); Scope scope_("ngw_walk_launch");
    const size_t n = (size_t)x->count, K = (size_t)x->K;
    rows_in(x->src, (size_t)x->rows, (size_t)x->S * (size_t)x->S, K);
    in(x->idx, n); in(x->items, n);
    out(x->dist, n * K, (int32_t)-1);
    if (x->items) { out(x->plans, (size_t)x->T * n, (int32_t)-1); out(x->length, n, (int32_t)-1); }
    flag_word(x->flags);
    return hipSuccess;
}

// ---------------------------------------------------------------- key tables: key[] / stamp[] / best[] / tag[] hold mask + 1 words
static void table_probe(const struct NgwTable* x, bool insert) {
    const size_t b = (size_t)(x->mask + 1), n = (size_t)x->count;
    in(x->keys, n);
    out(x->where, n, (int32_t)-1);
    if (insert) {
        inout(x->key, b); inout(x->stamp, b);
        inout(reinterpret_cast<uint64_t*>(x->stored), 1);
        flag_word(x->flags);
        out(x->fresh, n, (uint8_t)0);
    } else
        in(x->key, b);
}
hipError_t ngw_table_insert_launch(const struct NgwTable* x, hipStream_t) { HIT("ngw_table_insert_launch"); Scope scope_("ngw_table_insert_launch"); table_probe(x, true); return hipSuccess; }
hipError_t ngw_table_lookup_launch(const struct NgwTable* x, hipStream_t) { HIT("ngw_table_lookup_launch"); Scope scope_("ngw_table_lookup_launch"); table_probe(x, false); return hipSuccess; }
hipError_t ngw_table_insert_min_launch(const struct NgwTable* x, hipStream_t) { HIT("ngw_table_insert_min_launch"); Scope scope_("ngw_table_insert_min_launch");
    table_probe(x, true);
    const size_t b = (size_t)(x->mask + 1), n = (size_t)x->count;
    inout(x->best, b); inout(x->tag, b);
    in(x->values, n); in(x->tags, n);
    out(x->improved, n, (uint8_t)0);
    return hipSuccess;
}
hipError_t ngw_table_renorm_launch(uint64_t* best, uint64_t buckets, hipStream_t) { HIT("ngw_table_renorm_launch"); Scope scope_("ngw_table_renorm_launch"); inout(best, (size_t)buckets); return hipSuccess; }
hipError_t ngw_table_read_launch(const struct NgwTableRead* x, hipStream_t) { HIT("ngw_table_read_launch"); Scope scope_("ngw_table_read_launch");
    const size_t b = (size_t)(x->mask + 1), n = (size_t)x->count;
    in(x->best, b); in(x->tag, b); in(x->where, n);
    out(x->value, n, (int32_t)NGW_VALUE_NONE); out(x->tag_out, n, (int32_t)NGW_TAG_ROOT);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_table_trace_launch(const struct NgwTableTrace* x, hipStream_t) { HIT("ngw_table_trace_launch"); Scope scope_("ngw_table_trace_launch");
    const size_t b = (size_t)(x->mask + 1), n = (size_t)x->count;
    in(x->key, b); in(x->tag, b); in(x->where, n);
    out(x->plans, (size_t)x->T * n, (int32_t)-1); out(x->length, n, (int32_t)-1); out(x->root, n, (int32_t)-1);
    flag_word(x->flags);
    return hipSuccess;
}

// ---------------------------------------------------------------- frontiers and selections
hipError_t ngw_frontier_compact_launch(const struct NgwFrontier* x, hipStream_t) { HIT("ngw_frontier_compact_launch"); Scope scope_("ngw_frontier_compact_launch");
    in(x->bytes, (size_t)x->n);
    if (x->map) in(x->map, ceil_div(x->n, x->div));
    out(x->first, (size_t)x->capacity, (int32_t)NGW_IDX_NONE); out(x->second, (size_t)x->capacity, (int32_t)NGW_IDX_NONE);
    out(x->count, 2, (int32_t)0);
    inout(x->tiles, (size_t)x->n_tiles);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_frontier_alloc_launch(const struct NgwFrontierAlloc* x, hipStream_t) { HIT("ngw_frontier_alloc_launch"); Scope scope_("ngw_frontier_alloc_launch");
    in(x->count, 1);
    inout(x->cursor, 1);
    out(x->slots, (size_t)x->capacity, (int32_t)NGW_IDX_NONE);
    inout(x->ticket, 1);
    flag_word(x->flags);
    return hipSuccess;
}
hipError_t ngw_frontier_select_launch(const struct NgwSelect* x, hipStream_t) { HIT("ngw_frontier_select_launch"); Scope scope_("ngw_frontier_select_launch");
    const size_t g = (size_t)x->groups, all = g * (size_t)x->m;
    in(x->values, all); in(x->bytes, all);
    if (x->map) in(x->map, ceil_div((int64_t)all, x->div));
    out(x->first, (size_t)x->capacity, (int32_t)NGW_IDX_NONE); out(x->second, (size_t)x->capacity, (int32_t)NGW_IDX_NONE);
    out(x->taken, g, (int32_t)0); out(x->bound, g, (int32_t)NGW_VALUE_NONE);
    out(x->count, 2, (int32_t)0);
    // the wave form: the 64-bit ticket; the grid form: the state words, 8 words and 1024 counters per group, 2 * tiles_per_group tile words per group
    const size_t words = x->m <= NGW_SELECT_WAVE_MAX ? 2 : 4 + 8 * g + 1024 * g + 2 * g * (size_t)x->tiles_per_group;
    inout(x->scratch, words);
    return hipSuccess;
}

// ---------------------------------------------------------------- search runs: n = capacity * A positions
static size_t search_n(const struct NgwSearch* x) { return (size_t)x->capacity * (size_t)x->A; }
hipError_t ngw_search_take_launch(const struct NgwSearch* x, hipStream_t) { HIT("ngw_search_take_launch"); Scope scope_("ngw_search_take_launch");
    inout(const_cast<int32_t*>(x->parents), (size_t)x->capacity);
    inout(x->f, (size_t)x->pool);
    in(reinterpret_cast<const uint64_t*>(x->goal), 1);
    in(x->sel_count, 2);
    inout(x->orow, NGW_SEARCH_OPEN_COLS);
    return hipSuccess;
}
hipError_t ngw_search_open_launch(const struct NgwSearch* x, hipStream_t) { HIT("ngw_search_open_launch"); Scope scope_("ngw_search_open_launch");
    in(x->next, (size_t)x->capacity);
    if (x->dist) { in(x->dist, (size_t)x->capacity * (size_t)x->K); in(x->weights, (size_t)x->K); }
    in(x->g, (size_t)x->pool);
    inout(x->h, (size_t)x->pool); inout(x->f, (size_t)x->pool);
    return hipSuccess;
}
hipError_t ngw_search_offer_launch(const struct NgwSearch* x, hipStream_t) { HIT("ngw_search_offer_launch"); Scope scope_("ngw_search_offer_launch");
    const size_t n = search_n(x);
    in(x->parents, (size_t)x->capacity); in(x->g, (size_t)x->pool); in(x->bucket, (size_t)x->pool); in(x->info, n); in(x->lut, 64);
    out(x->values, n, (int32_t)NGW_VALUE_NONE); out(x->tags, n, (int32_t)NGW_TAG_ROOT);
    inout(x->row, 4);
    inout(reinterpret_cast<uint64_t*>(x->overflowed), 1);
    return hipSuccess;
}
hipError_t ngw_search_judge_launch(const struct NgwSearch* x, hipStream_t) { HIT("ngw_search_judge_launch"); Scope scope_("ngw_search_judge_launch");
    const size_t n = search_n(x);
    in(x->info, n); in(x->values, n); in(x->where, n);
    inout(x->best, n);
    inout(x->row, 4);
    inout(reinterpret_cast<uint64_t*>(x->goal), 1);
    return hipSuccess;
}
hipError_t ngw_search_settle_launch(const struct NgwSearch* x, hipStream_t) { HIT("ngw_search_settle_launch"); Scope scope_("ngw_search_settle_launch");
    const size_t n = search_n(x), cap = (size_t)x->capacity;
    in(x->first, cap); in(x->second, cap); in(x->slots, cap); in(x->parents, cap); in(x->values, n); in(x->where, n);
    out(x->plist, cap, (int32_t)NGW_IDX_NONE); out(x->next, cap, (int32_t)NGW_IDX_NONE);
    inout(x->g, (size_t)x->pool); inout(x->bucket, (size_t)x->pool);
    inout(x->row, 4); out(x->next_row, 4, 0u);
    if (x->f) {
        inout(x->f, (size_t)x->pool); inout(x->slot_of_bucket, (size_t)x->buckets);
        inout(x->orow, NGW_SEARCH_OPEN_COLS); inout(x->next_orow, NGW_SEARCH_OPEN_COLS);
    }
    return hipSuccess;
}
hipError_t ngw_search_roots_launch(const struct NgwSearchRoots* x, hipStream_t) { HIT("ngw_search_roots_launch"); Scope scope_("ngw_search_roots_launch");
    const size_t n = (size_t)x->count;
    in(x->roots, n); in(x->where, n); in(x->value, n); in(x->best, n);
    out(x->parents, (size_t)x->capacity, (int32_t)NGW_IDX_NONE);
    inout(x->g, (size_t)x->pool); inout(x->bucket, (size_t)x->pool);
    if (x->f) {
        inout(x->f, (size_t)x->pool); inout(x->h, (size_t)x->pool); inout(x->slot_of_bucket, (size_t)x->buckets);
        if (x->dist) { in(x->dist, n * (size_t)x->K); in(x->weights, (size_t)x->K); }
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- the recipe heuristic: map and inventory of [rows] rows, idx / out [count]
hipError_t ngw_recipe_launch(const struct NgwRecipe* x, hipStream_t) { HIT("ngw_recipe_launch"); Scope scope_("ngw_recipe_launch");
    const size_t rows = (size_t)x->rows, n = (size_t)x->count;
    if (x->prog.n_map) in(x->src.map, rows * (size_t)x->S2);   // "with n_map == 0 no map byte is read"
    in(x->src.inv, rows * (size_t)x->K);
    in(x->idx, n);                                     // (NULL: row j itself)
    out(x->out, n, (int32_t)0);
    flag_word(x->flags);
    return hipSuccess;
}

// ---------------------------------------------------------------- tree-search runs (the block comment above struct NgwTree): statistics [buckets][A]
// and [buckets]; recorded arrays step-major, n rows at `stride` with `count` live columns; touched [T][cap]; the leaves [count]; list [n_list]
static size_t tree_rec(const struct NgwTree* x) { return x->count ? (size_t)(x->n - 1) * (size_t)x->stride + (size_t)x->count : 0; }
static size_t tree_na(const struct NgwTree* x) { return (size_t)x->buckets * (size_t)x->A; }
hipError_t ngw_tree_leaf_launch(const struct NgwTree* x, hipStream_t) { HIT("ngw_tree_leaf_launch"); Scope scope_("ngw_tree_leaf_launch");
    const size_t n = (size_t)x->count;
    in(x->depth, n); in(x->length, n); in(x->keys, tree_rec(x)); in(x->masks, tree_rec(x));
    out(x->leaf_keys, n, (uint64_t)0); out(x->leaf_masks, n, (uint64_t)0);              // no pair has a leaf
    inout(x->row, NGW_TREE_COLS); out(x->next_row, NGW_TREE_COLS, 0u);
    return hipSuccess;
}
hipError_t ngw_tree_grow_launch(const struct NgwTree* x, hipStream_t) { HIT("ngw_tree_grow_launch"); Scope scope_("ngw_tree_grow_launch");
    const size_t n = (size_t)x->count;
    in(x->where_leaf, n); in(x->leaf_keys, n); in(x->leaf_masks, n); in(x->fresh, n);
    inout(x->mask_words, (size_t)x->buckets);
    inout(x->row, NGW_TREE_COLS);
    return hipSuccess;
}
static void tree_backup_touch(const struct NgwTree* x) {
    const size_t n = (size_t)x->count;
    in(x->actions, tree_rec(x)); in(x->rewards, tree_rec(x)); in(x->where, tree_rec(x));
    in(x->depth, n); in(x->length, n); in(x->bootstrap, n); in(x->where_leaf, n);       // (bootstrap, where_leaf: NULL = none)
    inout(x->visits, tree_na(x)); inout(x->returns, tree_na(x));
    out(x->touched, (size_t)x->T * (size_t)x->cap, (int32_t)-1);                        // also the lanes count <= j < cap: nothing touched
    inout(x->row, NGW_TREE_COLS);
}
static void tree_reweight_touch(const struct NgwTree* x) {
    in(x->list, (size_t)x->n_list);
    in(x->visits, tree_na(x)); in(x->returns, tree_na(x)); in(x->mask_words, (size_t)x->buckets); in(x->priors, tree_na(x));
    inout(x->rows, tree_na(x));
    flag_word(x->flags);
}
hipError_t ngw_tree_backup_launch(const struct NgwTree* x, hipStream_t) { HIT("ngw_tree_backup_launch"); Scope scope_("ngw_tree_backup_launch"); tree_backup_touch(x); return hipSuccess; }
hipError_t ngw_tree_backup_discount_launch(const struct NgwTree* x, const struct NgwTreeRule* r, hipStream_t) { HIT("ngw_tree_backup_discount_launch"); Scope scope_("ngw_tree_backup_discount_launch");
    in(r, 1); tree_backup_touch(x);
    return hipSuccess;
}
hipError_t ngw_tree_reweight_launch(const struct NgwTree* x, hipStream_t) { HIT("ngw_tree_reweight_launch"); Scope scope_("ngw_tree_reweight_launch"); tree_reweight_touch(x); return hipSuccess; }
hipError_t ngw_tree_reweight16_launch(const struct NgwTree* x, const struct NgwTreeRule* r, hipStream_t) { HIT("ngw_tree_reweight16_launch"); Scope scope_("ngw_tree_reweight16_launch");
    in(r, 1); tree_reweight_touch(x);
    return hipSuccess;
}

}  // extern "C"
