// main.cpp - the scenarios of the host-side sanitizer harness.  Usage:
//     hostcheck <scenario> <spec file> [<spec file> ...] [short=<allocation>]      (refusals: the second spec file is a 36 x 36 map, the third 48 x 48)
// A spec file holds the bytes of one compiled ngw_spec (its length is checked against ngw_spec_size()).  The program drives the public C-ABI
// (include/ngw.h) only, against the fake HIP runtime and the launch stubs it is linked with; every buffer it hands in is a heap block of exactly
// the documented size, so AddressSanitizer sees the first byte a call reads or writes past it.  After each handle's ngw_destroy the fake's
// ledger must be empty.  A scenario that a sanitizer or the ledger objects to ends the program non-zero and names itself.
// short=<allocation> (the -DFAKE_HIP_SHORT build): only that allocation is handed out short - the harness's proof that it can fail.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/ngw.h"

namespace {

const char* g_scenario = "?";
std::string g_short;            // the allocation to hand out short, or empty
bool g_short_armed = false;
std::vector<std::vector<uint8_t>> g_specs;

[[noreturn]] void die(int line, const char* what) {
    fprintf(stderr, "hostcheck: scenario '%s' FAILED at main.cpp:%d: %s (ngw_last_error: %s)\n", g_scenario, line, what, ngw_last_error());
    exit(1);
}
#define OK(expr) do { if ((expr) != NGW_OK) die(__LINE__, #expr " did not return NGW_OK"); } while (0)
#define REQUIRE(cond) do { if (!(cond)) die(__LINE__, "required: " #cond); } while (0)

// the allocation the next C-ABI call makes is the one named `name`: handed out short if the command line picked it
void arm(const char* name) {
    if (g_short != name || g_short_armed) return;
    g_short_armed = true;
    fake_hip_short_only(0);
}

// an exact-size heap block ("device" memory is heap memory under the fake)
struct Buf {
    void* p;
    size_t bytes;
    explicit Buf(size_t b, int fill = 0) : p(malloc(b ? b : 1)), bytes(b) { if (b) memset(p, fill, b); }
    Buf(const Buf&) = delete;
    ~Buf() { free(p); }
    template <typename T> T* as() { return static_cast<T*>(p); }
};
template <typename T> struct Arr : Buf {
    explicit Arr(size_t n, T v = T()) : Buf(n * sizeof(T)) { for (size_t i = 0; i < n; i++) get()[i] = v; }
    T* get() { return static_cast<T*>(p); }
    operator T*() { return get(); }
};
Arr<int32_t>* iota_list(size_t n, int32_t step = 1) {
    auto* a = new Arr<int32_t>(n);
    for (size_t i = 0; i < n; i++) (*a)[i] = (int32_t)i * step;
    return a;
}

const ngw_spec* spec(size_t i = 0) { return reinterpret_cast<const ngw_spec*>(g_specs[i % g_specs.size()].data()); }

void ledger_empty(int line) {
    if (fake_hip_live_total() == 0) return;
    fake_hip_report();
    die(line, "the ledger is not empty after ngw_destroy: something was never released");
}
#define DESTROY(h) do { OK(ngw_destroy(h)); ledger_empty(__LINE__); } while (0)

ngw_handle* make(const ngw_spec* sp, int64_t n, int autoreset = 0) {
    ngw_handle* h = nullptr;
    OK(ngw_create(sp, n, 0, 1234, 0, &h));
    REQUIRE(h != nullptr);
    OK(ngw_set_autoreset(h, autoreset, 0));
    OK(ngw_reset(h, nullptr));
    return h;
}

const int64_t ENVS[5] = {1, 63, 64, 65, 130};

// ---------------------------------------------------------------- handle
void scenario_handle() {
    const ngw_spec* sp = spec();
    const size_t S2 = (size_t)sp->map_size * sp->map_size, K = (size_t)sp->n_items;
    for (int64_t n : ENVS)
        for (int ar = 0; ar < 2; ar++) {
            ngw_handle* h = make(sp, n, ar);
            const size_t N = (size_t)n;
            Arr<uint8_t> mask(N, 1);
            OK(ngw_reset(h, mask));
            OK(ngw_reset(h, mask));                      // (the second half of the page-locked mask buffer)
            Arr<int32_t> actions(N, 0);
            OK(ngw_step(h, actions));
            OK(ngw_step(h, actions));
            {   // state out and in, every array exactly as long as documented; a sub-range too
                Arr<int8_t> map(N * S2); Arr<int32_t> loc(N * 2), facing(N), inv(N * K), sel(N), stp(N); Arr<uint32_t> epi(N);
                OK(ngw_get_state(h, 0, n, map, loc, facing, inv, sel, stp, epi));
                Arr<int8_t> map2(N * S2, 1); Arr<int32_t> loc2(N * 2, 1), facing2(N, 3), inv2(N * K, 7), sel2(N, 2), stp2(N, 5); Arr<uint32_t> epi2(N, 9u);
                OK(ngw_set_state(h, 0, n, map2, loc2, facing2, inv2, sel2, stp2, epi2));
                OK(ngw_get_state(h, 0, n, map, loc, facing, inv, sel, stp, epi));
                REQUIRE(!memcmp(map.p, map2.p, map.bytes) && !memcmp(loc.p, loc2.p, loc.bytes) && !memcmp(inv.p, inv2.p, inv.bytes));
                REQUIRE(!memcmp(sel.p, sel2.p, sel.bytes) && !memcmp(stp.p, stp2.p, stp.bytes) && !memcmp(epi.p, epi2.p, epi.bytes));
                const int64_t first = n - 1;
                Arr<int8_t> m1(S2); Arr<int32_t> l1(2), f1(1), i1(K), s1(1), t1(1); Arr<uint32_t> e1(1);
                OK(ngw_get_state(h, first, 1, m1, l1, f1, i1, s1, t1, e1));
                OK(ngw_set_state(h, first, 1, m1, l1, f1, i1, s1, t1, e1));
                OK(ngw_get_state(h, 0, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
                Arr<int8_t> om(N * S2); Arr<int32_t> ol(N * 2), of(N), oi(N * K);
                OK(ngw_get_obs(h, om, ol, of, oi));
                Arr<int32_t> rw(N); Arr<uint8_t> dn(N), rs(N), cc(N); Arr<uint16_t> mc(N), ma(N);
                OK(ngw_get_step_out(h, rw, dn, rs, cc, mc, ma));
                uint32_t flags = 1;
                OK(ngw_error_flags(h, &flags));
            }
            // prepared next episodes at depth 1 and 2 with terminal capture, steps and a refill behind them, then destroy
            OK(ngw_set_terminal_capture(h, 1));
            for (int depth = 1; depth <= 2; depth++) {
                OK(ngw_set_reset_prefetch_depth(h, depth));
                OK(ngw_set_reset_prefetch(h, 2));
                for (int i = 0; i < 5; i++) OK(ngw_step(h, actions));
                OK(ngw_reset(h, nullptr));
                Arr<int8_t> tm(N * S2); Arr<int32_t> tl(N * 2), tf(N), ti(N * K);
                OK(ngw_get_terminal_obs(h, tm, tl, tf, ti));
            }
            // a captured graph of two steps, replayed, left for ngw_destroy to drop
            Arr<int32_t> dev_actions(2 * N, 0);
            OK(ngw_graph_build(h, dev_actions, n, 2));
            OK(ngw_graph_launch(h, 2));
            OK(ngw_stream_order(h, nullptr, 1));
            DESTROY(h);
        }
}

// ---------------------------------------------------------------- host_step
void lidar_on(ngw_handle* h, const ngw_spec* sp, int bits) {
    static ngw_lidar_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.num_beams = 8; cfg.max_range = 11; cfg.n_chan = sp->n_items - 2; cfg.n_inv = sp->n_items;
    for (int i = 1; i <= cfg.n_chan; i++) cfg.chan_of_item[i] = (uint8_t)i;
    for (int i = 0; i < cfg.n_inv; i++) cfg.inv_item[i] = (uint8_t)i;
    OK(ngw_lidar_configure(h, &cfg));
    OK(ngw_lidar_set_output(h, bits));
    OK(ngw_lidar_fuse(h, 1));
}

void host_step_once(const ngw_spec* sp, int64_t n, int lidar_bits) {
    const size_t N = (size_t)n, S2 = (size_t)sp->map_size * sp->map_size, K = (size_t)sp->n_items;
    ngw_handle* h = make(sp, n, 1);
    int32_t row_bytes = 0;
    void* rows = nullptr;
    if (lidar_bits) {
        lidar_on(h, sp, lidar_bits);
        OK(ngw_lidar_row_layout(h, &row_bytes, nullptr, nullptr, nullptr));
        rows = ngw_host_alloc((uint64_t)((N + 63) / 64 * 64) * (uint64_t)row_bytes);      // ([n_pad] rows: ngw_device.h NgwWT::rows)
        REQUIRE(rows != nullptr);
        OK(ngw_lidar_host_rows(h, rows));
    }
    Arr<int32_t> actions(N, 0);
    {   // separate arrays, each exactly as long as documented; then each optional output NULL in turn
        Arr<int8_t> map(N * S2); Arr<int32_t> loc(N * 2), facing(N), inv(N * K), reward(N), stp(N);
        Arr<uint8_t> done(N), result(N), cost(N), sel(N); Arr<uint16_t> mc(N), ma(N);
        uint32_t* flags = static_cast<uint32_t*>(malloc(4));
        for (int rep = 0; rep < 2; rep++)
            OK(ngw_step_host(h, actions, map, loc, facing, inv, reward, done, result, cost, mc, ma, flags, sel, stp));
        for (int skip = 0; skip < 13; skip++) {
            auto P = [&](int i, auto* p) { return i == skip ? decltype(p)(nullptr) : p; };
            OK(ngw_step_host(h, actions, P(0, map.get()), P(1, loc.get()), P(2, facing.get()), P(3, inv.get()), P(4, reward.get()), P(5, done.get()),
                             P(6, result.get()), P(7, cost.get()), P(8, mc.get()), P(9, ma.get()), P(10, flags), P(11, sel.get()), P(12, stp.get())));
        }
        OK(ngw_step_host(h, actions, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        free(flags);
        if (lidar_bits) { Buf lr(N * (size_t)row_bytes); OK(ngw_get_lidar(h, lr.p)); }
    }
    {   // the one-block layout: the sections of one page-locked block of exactly offsets11[10] bytes, kept from call to call
        uint64_t off[11];
        OK(ngw_host_step_layout(h, off));
        uint8_t* b = static_cast<uint8_t*>(ngw_host_alloc(off[10]));
        REQUIRE(b != nullptr);
        Arr<uint8_t> result(N);
        for (int rep = 0; rep < 4; rep++) {
            if (rep == 3) OK(ngw_host_mirror_invalidate(h));
            OK(ngw_step_host(h, actions, reinterpret_cast<int8_t*>(b + off[0]), reinterpret_cast<int32_t*>(b + off[1]), reinterpret_cast<int32_t*>(b + off[2]),
                             reinterpret_cast<int32_t*>(b + off[3]), reinterpret_cast<int32_t*>(b + off[4]), b + off[5], result, nullptr, nullptr, nullptr,
                             reinterpret_cast<uint32_t*>(b + off[7]), b + off[8], reinterpret_cast<int32_t*>(b + off[9])));
        }
        OK(ngw_host_free(b));
    }
    {   // the narrow wire format: a block of exactly offsets8[7] bytes; first call (full copy, shadows seeded), the steady state, without the map,
        // after something else wrote the state, and a bad action id in the middle of the batch
        uint64_t off[8];
        OK(ngw_host_step_layout_packed(h, off));
        void* b = ngw_host_alloc(off[7]);
        REQUIRE(b != nullptr);
        for (int rep = 0; rep < 4; rep++) OK(ngw_step_host_packed(h, actions, b, rep != 2));
        OK(ngw_reset(h, nullptr));
        for (int rep = 0; rep < 3; rep++) OK(ngw_step_host_packed(h, actions, b, 1));
        actions[N / 2] = sp->n_actions;
        REQUIRE(ngw_step_host_packed(h, actions, b, 1) == NGW_E_INVALID_ACTION);
        actions[N / 2] = 0;
        actions[N - 1] = -1;
        REQUIRE(ngw_step_host_packed(h, actions, b, 1) == NGW_E_INVALID_ACTION);
        REQUIRE(ngw_step_host(h, actions, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
                NGW_E_INVALID_ACTION);
        actions[N - 1] = 0;
        OK(ngw_step_host_packed(h, actions, b, 1));
        void* pageable = malloc(off[7]);                 // a block the GPU cannot address: full copies every time
        for (int rep = 0; rep < 2; rep++) OK(ngw_step_host_packed(h, actions, pageable, 1));
        free(pageable);
        OK(ngw_host_free(b));
    }
    {   // ngw_reset_host into exact-size arrays
        Arr<int8_t> map(N * S2); Arr<int32_t> loc(N * 2), facing(N), inv(N * K), stp(N); Arr<uint8_t> sel(N);
        uint32_t flags = 0;
        OK(ngw_reset_host(h, nullptr, map, loc, facing, inv, sel, stp, &flags));
        Arr<uint8_t> mask(N, 1);
        OK(ngw_reset_host(h, mask, map, loc, facing, inv, sel, stp, &flags));
    }
    if (rows) { OK(ngw_lidar_host_rows(h, nullptr)); OK(ngw_host_free(rows)); }
    DESTROY(h);
}

void scenario_host_step() {
    const ngw_spec* sp = spec();
    const char* const onoff[2] = {"0", "1"};
    for (int delta = 0; delta < 2; delta++)
        for (int wt = 0; wt < 2; wt++) {
            setenv("NGW_HOST_DELTA", onoff[delta], 1);
            setenv("NGW_HOST_WRITE_THROUGH", onoff[wt], 1);
            for (int zc = 0; zc < 2; zc++) {             // the small-batch mapped-block path, then the staged one
                if (zc) setenv("NGW_ZC_BYTES", "1", 1); else unsetenv("NGW_ZC_BYTES");
                for (int64_t n : ENVS) host_step_once(sp, n, 0);
            }
        }
    // lidar rows in the three formats riding along (the staged path: the one-block and the wire forms run)
    const int bits[3] = {32, 16, 8};
    for (int b : bits)
        for (int64_t n : {(int64_t)64, (int64_t)65, (int64_t)128}) host_step_once(sp, n, b);
    unsetenv("NGW_ZC_BYTES"); unsetenv("NGW_HOST_DELTA"); unsetenv("NGW_HOST_WRITE_THROUGH");
}

// ---------------------------------------------------------------- snapshot
void scenario_snapshot() {
    const ngw_spec* sp = spec();
    const size_t S2 = (size_t)sp->map_size * sp->map_size, K = (size_t)sp->n_items, A = (size_t)sp->n_actions;
    const int64_t n = 130;
    ngw_handle* h = make(sp, n);
    const int64_t caps[4] = {64, 1, 65, 4096};
    for (int64_t cap : caps) {
        ngw_snapshot *s = nullptr, *s2 = nullptr;
        if (cap == 64) arm("snapshot_slab");
        if (cap == 65) arm("snapshot_slab_padded");
        OK(ngw_snapshot_create(h, cap, &s));
        OK(ngw_snapshot_create(h, cap, &s2));
        const int64_t counts[6] = {0, 1, 63, 64, 65, cap};
        for (int64_t c : counts) {
            if (c > cap) continue;
            const size_t C = (size_t)c;
            const int64_t ce = c < n ? c : n;            // (a list of envs: at most n of them)
            Arr<int32_t>* idx = iota_list(C);
            Arr<int32_t>* env_idx = iota_list((size_t)ce);
            OK(ngw_snapshot_save(h, s, *env_idx, *idx, ce));
            OK(ngw_snapshot_save(h, s, nullptr, nullptr, ce));
            OK(ngw_snapshot_restore(h, s, *idx, *env_idx, ce, 0));
            OK(ngw_snapshot_restore(h, s, nullptr, nullptr, ce, NGW_SNAP_KEEP_EPISODE));
            OK(ngw_snapshot_copy(h, s, *idx, s2, *idx, c));
            OK(ngw_snapshot_copy(h, s, nullptr, s2, nullptr, c));
            {
                Arr<int32_t> actions(C, 0), reward(C); Arr<uint8_t> done(C); Arr<uint32_t> info(C);
                OK(ngw_snapshot_expand(h, s, *idx, actions, s2, *idx, c, reward, done, info));
                OK(ngw_snapshot_expand(h, nullptr, *env_idx, actions, s2, nullptr, ce, nullptr, nullptr, nullptr));
            }
            {
                Arr<uint64_t> keys(C), skeys(C * A); Arr<int32_t> reward(C * A); Arr<uint8_t> done(C * A); Arr<uint32_t> info(C * A);
                OK(ngw_state_keys(h, s, *idx, c, NGW_KEY_STATE, keys));
                OK(ngw_state_keys(h, nullptr, nullptr, ce, NGW_KEY_ALL, keys));
                OK(ngw_successor_keys(h, s, *idx, c, NGW_KEY_STATE, skeys, reward, done, info));
                OK(ngw_successor_keys(h, s, nullptr, c, NGW_KEY_STATE, skeys, nullptr, nullptr, nullptr));
            }
            {
                const int T = 7;
                Arr<int32_t> dist(C * K), items(C, 1), plans((size_t)T * C), length(C);
                OK(ngw_snapshot_walk(h, s, *idx, c, nullptr, 0, dist, nullptr, nullptr));
                OK(ngw_snapshot_walk(h, s, *idx, c, items, T, dist, plans, length));
                OK(ngw_snapshot_walk(h, s, nullptr, c, items, T, nullptr, plans, length));
            }
            {
                Arr<int8_t> map(C * S2); Arr<int32_t> loc(C * 2), facing(C), inv(C * K), sel(C), stp(C); Arr<uint32_t> epi(C);
                OK(ngw_snapshot_get(h, s, 0, c, map, loc, facing, inv, sel, stp, epi));
                if (c) OK(ngw_snapshot_get(h, s, cap - c, c, map, loc, facing, inv, sel, stp, epi));
                Arr<uint64_t> masks(C);
                OK(ngw_snapshot_action_mask(h, s, *idx, c, masks));
            }
            delete idx; delete env_idx;
        }
        if (cap != 4096) { OK(ngw_snapshot_destroy(h, s)); OK(ngw_snapshot_destroy(h, s2)); }     // (the last two stay open: ngw_destroy's to release)
    }
    DESTROY(h);
}

// ---------------------------------------------------------------- table
void scenario_table() {
    const ngw_spec* sp = spec();
    ngw_handle* h = make(sp, 65);
    const int64_t caps[5] = {1, 3, 4, 1024, 1025}, counts[6] = {0, 1, 63, 64, 65, 600};
    ngw_key_table* left_open = nullptr;
    for (int valued = 0; valued < 2; valued++)
        for (int64_t cap : caps) {
            ngw_key_table* t = nullptr;
            arm(valued ? "table_slab_valued" : "table_slab_plain");
            if (valued) OK(ngw_key_table_create_valued(h, cap, 0, &t)); else OK(ngw_key_table_create(h, cap, &t));
            for (int64_t c : counts) {
                const size_t C = (size_t)c;
                Arr<uint64_t> keys(C, 77); Arr<int32_t> where(C), values(C, 3), tags(C, -1), value(C), tag(C), length(C), root(C); Arr<uint8_t> fresh(C), best(C);
                OK(ngw_key_table_insert(h, t, keys, c, where, fresh));
                OK(ngw_key_table_lookup(h, t, keys, c, where));
                if (valued) {
                    OK(ngw_key_table_insert_min(h, t, keys, values, tags, c, where, fresh, best));
                    OK(ngw_key_table_insert_min(h, t, keys, values, nullptr, c, where, fresh, best));
                    OK(ngw_key_table_read(h, t, where, c, value, tag));
                    for (int T : {0, 1, 7}) {
                        Arr<int32_t> plans((size_t)T * C);
                        OK(ngw_key_table_trace(h, t, where, c, T, sp->n_actions, T ? plans.get() : nullptr, length, root));
                    }
                }
                int64_t stored = -1;
                OK(ngw_key_table_count(h, t, &stored));
                REQUIRE(stored == 0);                    // (the stubs store nothing)
            }
            OK(ngw_key_table_clear(h, t));
            if (valued && cap == 1025) left_open = t; else OK(ngw_key_table_destroy(h, t));
        }
    {   // the renormalising pass inside a call: the low half of the positions would wrap in the first call of 600
        ngw_key_table* t = nullptr;
        OK(ngw_key_table_create_valued(h, 64, (1ull << 32) - 100, &t));
        for (int rep = 0; rep < 3; rep++) {
            const size_t C = 600;
            Arr<uint64_t> keys(C, 5); Arr<int32_t> where(C), values(C, 3); Arr<uint8_t> fresh(C), best(C);
            OK(ngw_key_table_insert_min(h, t, keys, values, nullptr, (int64_t)C, where, fresh, best));
            OK(ngw_key_table_insert(h, t, keys, (int64_t)C, where, fresh));
        }
        OK(ngw_key_table_destroy(h, t));
    }
    REQUIRE(left_open != nullptr);
    DESTROY(h);
}

// ---------------------------------------------------------------- frontier
void select_call(ngw_handle* h, int64_t m, int32_t groups, bool with_flags, bool with_second) {
    const size_t all = (size_t)(m * groups), keep = m < 3 ? (size_t)m : 3, cap = (size_t)groups * keep;
    Arr<int32_t> values(all, 5), first(cap), second(cap), taken((size_t)groups), bound((size_t)groups), count(2);
    Arr<uint8_t> flags(all, 1);
    OK(ngw_frontier_select(h, values, with_flags ? flags.get() : nullptr, (int64_t)all, groups, 1, nullptr, (int32_t)keep, 0, (int64_t)cap, first,
                           with_second ? second.get() : nullptr, taken, bound, count));
    Arr<int32_t> map((all + 6) / 7);                     // div 7 with a map of exactly ceil(n / div) entries
    OK(ngw_frontier_select(h, values, nullptr, (int64_t)all, groups, 7, map, (int32_t)keep, 1, (int64_t)cap, first, second, taken, bound, count));
}

void scenario_frontier() {
    const ngw_spec* sp = spec();
    ngw_handle* h = make(sp, 65);
    bool first_compact = true;
    const int64_t ns[8] = {0, 1, 4095, 4096, 4097, 513 * 4096 + 1, 5, 514 * 4096};   // past the 512-tile floor (regrow), a small one after it (none), a larger one (regrow)
    for (int64_t n : ns) {
        const size_t N = (size_t)n, cap = 100;
        Arr<uint8_t> flags(N, 1); Arr<int32_t> first(cap), second(cap), count(2), map((N + 2) / 3);
        if (first_compact) { arm("frontier_scratch"); first_compact = false; }
        if (n == 513 * 4096 + 1) arm("frontier_scratch_regrown");          // (514 tiles: the ticket + 514 counts, exactly)
        OK(ngw_frontier_compact(h, flags, n, 1, nullptr, (int64_t)cap, first, second, count));
        OK(ngw_frontier_compact(h, flags, n, 3, map, (int64_t)cap, first, nullptr, count));
        OK(ngw_frontier_compact(h, flags, n, 3, nullptr, 0, nullptr, nullptr, count));
        Arr<int32_t> cursor(1), slots(cap);
        OK(ngw_frontier_alloc(h, count, cursor, 1000, (int64_t)cap, slots));
        OK(ngw_frontier_alloc(h, count, cursor, 1000, 0, nullptr));
    }
    arm("select_scratch");
    for (int64_t m : {(int64_t)1, (int64_t)1023, (int64_t)1024})                      // the wave form
        for (int32_t g : {1, 3, 65}) select_call(h, m, g, g != 3, g != 1);
    for (int64_t m : {(int64_t)1025, (int64_t)4096, (int64_t)4097, (int64_t)(3 * 4096 + 5)})   // the grid form
        for (int32_t g : {1, 3}) select_call(h, m, g, g == 3, true);
    arm("select_scratch_regrown");
    select_call(h, 1025, 4, false, false);               // 4 + 1032 * 4 + 2 * 4 = 4140 words: past the 4096-word floor (regrow)
    select_call(h, 1025, 1, true, true);                 // a small call after a large one (no regrow)
    select_call(h, 4097, 8, true, false);                // a larger one (regrow)
    DESTROY(h);
}

// ---------------------------------------------------------------- search
void search_reads(ngw_handle* h, ngw_search* s, bool open) {
    auto* rep = static_cast<ngw_search_report*>(malloc(sizeof(ngw_search_report)));
    OK(ngw_search_read(h, s, rep));
    REQUIRE(rep->rows >= 0 && rep->rows <= NGW_SEARCH_ROWS);
    free(rep);
    if (open) {
        auto* orep = static_cast<ngw_search_open_report*>(malloc(sizeof(ngw_search_open_report)));
        OK(ngw_search_read_open(h, s, orep));
        free(orep);
    }
}

void search_drive(ngw_handle* h, ngw_search* s, int64_t cap, bool open, bool long_run) {
    int32_t cur = -1;
    for (int64_t roots : {(int64_t)0, (int64_t)1, cap}) {
        Arr<int32_t>* r = iota_list((size_t)roots);
        OK(ngw_search_start(h, s, roots ? r->get() : nullptr, roots, &cur));
        delete r;
        OK(ngw_search_run(h, s, 1, &cur));
        search_reads(h, s, open);
    }
    if (long_run) { OK(ngw_search_run(h, s, 66, nullptr)); search_reads(h, s, open); }   // (the stats ring of 65 rows, past its wrap)
    OK(ngw_search_run(h, s, 0, &cur));
}

void scenario_search() {
    int32_t costs[64];
    for (int i = 0; i < 64; i++) costs[i] = 1;
    for (size_t si = 0; si < g_specs.size(); si++) {
        const ngw_spec* sp = spec(si);
        ngw_handle* h = make(sp, 65);
        const int32_t K = sp->n_items;
        Arr<int32_t> weights((size_t)K, 1);
        const int64_t pools[3] = {64, 65, 4097}, caps[5] = {1, 2, 3, 64, 65}, tcaps[2] = {64, 1000};
        for (int64_t pc : pools) {
            ngw_snapshot* pool = nullptr;
            OK(ngw_snapshot_create(h, pc, &pool));
            for (int64_t tc : tcaps) {
                ngw_key_table* table = nullptr;
                OK(ngw_key_table_create_valued(h, tc, 0, &table));
                for (int64_t cap : caps) {
                    if (cap > pc) continue;
                    const bool long_run = pc == 64 && tc == 64;
                    ngw_search* s = nullptr;
                    ngw_search_arrays arr;
                    if (si == 0 || long_run)
                        for (int32_t keep : {-1, 1, (int32_t)cap}) {
                            arm("search_slab_closed");
                            OK(ngw_search_create(h, pool, table, cap, costs, keep == 1, keep, keep == 1, &arr, &s));
                            search_drive(h, s, cap, false, long_run && keep == -1);
                            OK(ngw_search_destroy(h, s));
                        }
                    ngw_search_options o;
                    memset(&o, 0, sizeof(o));
                    o.capacity = cap; o.costs_host = costs; o.keep = 1; o.prune = 1;
                    ngw_search_arrays_open oarr;
                    if (si == 0 || long_run) {
                        OK(ngw_search_create_open(h, pool, table, &o, &oarr, &s));          // no heuristic
                        search_drive(h, s, cap, true, false);
                        OK(ngw_search_destroy(h, s));
                    }
                    for (int32_t mode : {NGW_SEARCH_H_MIN, NGW_SEARCH_H_MAX}) {            // the walk heuristic: weights and distances in the slab
                        o.heuristic = mode; o.n_weights = K; o.weights_host = weights; o.keep = mode == NGW_SEARCH_H_MIN ? 1 : (int32_t)cap;
                        arm("search_slab_open");
                        OK(ngw_search_create_open(h, pool, table, &o, &oarr, &s));
                        search_drive(h, s, cap, true, long_run && mode == NGW_SEARCH_H_MIN);
                        OK(ngw_search_destroy(h, s));
                    }
                }
                if (tc == 1000 && pc == 4097) {
                    // a search whose table is closed first: every call but destroy refuses it; then it stays open for ngw_destroy
                    ngw_search* s = nullptr;
                    ngw_search_arrays arr;
                    OK(ngw_search_create(h, pool, table, 3, costs, 0, -1, 0, &arr, &s));
                    OK(ngw_key_table_destroy(h, table));
                    REQUIRE(ngw_search_run(h, s, 1, nullptr) == NGW_E_INVALID_ARG);
                    REQUIRE(ngw_search_start(h, s, nullptr, 0, nullptr) == NGW_E_INVALID_ARG);
                    search_reads(h, s, false);
                } else
                    OK(ngw_key_table_destroy(h, table));
            }
            if (pc != 4097) OK(ngw_snapshot_destroy(h, pool));
        }
        DESTROY(h);
    }
}

// ---------------------------------------------------------------- tree
// the staged calls over the caller's own arrays of a guided playout: step-major, `stride` > count apart, n_steps rows - each exactly that long
void tree_stages(ngw_handle* h, ngw_tree* t, int64_t P, int32_t T) {
    const int64_t count = P, stride = P + 3;
    const int32_t n = T > 1 ? T - 1 : 1;
    const size_t C = (size_t)count, rec = (size_t)(n - 1) * (size_t)stride + C;
    Arr<int32_t> depth(C, 1), length(C, n), actions(rec, 0), rewards(rec, 1), where(rec, -1), bootstrap(C, 2), buckets(C, 0);
    Arr<uint64_t> keys(rec, 7), masks(rec, 1);
    OK(ngw_tree_grow(h, t, depth, length, keys, masks, stride, count, n));
    for (int use_leaves = 0; use_leaves < 2; use_leaves++)
        for (int boot = 0; boot < 2; boot++)
            OK(ngw_tree_backup(h, t, actions, rewards, where, depth, length, stride, count, n, use_leaves, boot ? bootstrap.get() : nullptr));
    OK(ngw_tree_reweight(h, t, nullptr, 0));
    OK(ngw_tree_reweight(h, t, buckets, count));
    OK(ngw_tree_grow(h, t, nullptr, nullptr, nullptr, nullptr, 0, 0, 1));            // no pairs: only the leaves are forgotten
}

void tree_report(ngw_handle* h, ngw_tree* t) {
    auto* rep = static_cast<ngw_tree_report_rows*>(malloc(sizeof(ngw_tree_report_rows)));
    OK(ngw_tree_report(h, t, rep));
    REQUIRE(rep->rows >= 0 && rep->rows <= NGW_TREE_ROWS);
    free(rep);
}

void scenario_tree() {
    // (spread, discount_q16, rows16): both reweight kernels and both backup kernels, rows16 = 2 at spread 1 only
    const ngw_tree_rule rules[8] = {{1, 65536, 1, 0}, {1, 65536, 2, 0}, {1, 32768, 0, 0}, {16, 65536, 0, 0}, {16, 32768, 1, 0}, {64, 32768, 0, 0}, {64, 65536, 1, 0},
                                    {1, 65536, 0, 0}};
    for (size_t si = 0; si < g_specs.size(); si++) {
        const ngw_spec* sp = spec(si);
        const int64_t n = 65;
        ngw_handle* h = make(sp, n);
        Arr<float> weights((size_t)sp->n_actions, 1.0f);
        ngw_snapshot* snap = nullptr;
        OK(ngw_snapshot_create(h, n, &snap));
        OK(ngw_snapshot_save(h, snap, nullptr, nullptr, n));
        for (int64_t tc : {(int64_t)64, (int64_t)1000}) {
            ngw_key_table* table = nullptr;
            OK(ngw_key_table_create(h, tc, &table));
            for (int64_t P : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65})
                for (int32_t T : {1, 2, 5})
                    for (int priors = 0; priors < 2; priors++)
                        for (int given = 0; given < 2; given++) {
                            ngw_tree_options o;
                            memset(&o, 0, sizeof(o));
                            o.playouts = P; o.steps = T; o.fields = NGW_KEY_STATE; o.c = 1.0f; o.q_init = 0.0f; o.priors = priors;
                            o.weights_host = given ? weights.get() : nullptr;
                            ngw_tree* t = nullptr;
                            if (P == 1 && T == 1 && tc == 64 && !priors && !given) arm("tree_slab");
                            OK(ngw_tree_create(h, table, &o, &t));
                            ngw_tree_device_arrays arr;
                            OK(ngw_tree_arrays(h, t, &arr));
                            REQUIRE(arr.n_actions == sp->n_actions && (arr.priors != nullptr) == (priors != 0));
                            Arr<int32_t>* roots = iota_list((size_t)P);
                            for (ngw_snapshot* src : {snap, (ngw_snapshot*)nullptr}) {     // count == P roots: the last byte of fresh[] is touched
                                OK(ngw_tree_start(h, t, src, *roots, P));
                                OK(ngw_tree_run(h, t, 1, 5));
                                tree_report(h, t);
                            }
                            for (const ngw_tree_rule& r : rules) {
                                OK(ngw_tree_set_rule(h, t, &r));
                                OK(ngw_tree_run(h, t, 1, 5));
                                if (P == 64 || T == 5) tree_stages(h, t, P, T);           // (the staged backup and reweight under the rule too)
                            }
                            tree_stages(h, t, P, T);
                            if (P == 65 && T == 2 && !priors && given) { OK(ngw_tree_run(h, t, NGW_TREE_ROWS + 2, 5)); tree_report(h, t); }   // (the stats ring, past its wrap)
                            OK(ngw_tree_clear(h, t));
                            OK(ngw_tree_run(h, t, 1, 6));                                  // (no roots)
                            OK(ngw_tree_start(h, t, nullptr, *roots, P));
                            OK(ngw_tree_run(h, t, 1, 6));
                            tree_report(h, t);
                            delete roots;
                            OK(ngw_tree_destroy(h, t));
                        }
            if (tc == 1000) {
                // a tree whose table is closed first: every call that needs the table refuses it; then it stays open for ngw_destroy
                ngw_tree_options o;
                memset(&o, 0, sizeof(o));
                o.playouts = 3; o.steps = 2; o.fields = NGW_KEY_STATE; o.c = 1.0f;
                ngw_tree* t = nullptr;
                OK(ngw_tree_create(h, table, &o, &t));
                OK(ngw_key_table_destroy(h, table));
                Arr<int32_t> i32(8, 0); Arr<uint64_t> u64(8, 0);
                const ngw_tree_rule rule = {1, 65536, 0, 0};
                REQUIRE(ngw_tree_run(h, t, 1, 0) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_start(h, t, nullptr, nullptr, 0) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_grow(h, t, i32, i32, u64, u64, 3, 3, 1) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_backup(h, t, i32, i32, i32, i32, i32, 3, 3, 1, 0, nullptr) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_reweight(h, t, nullptr, 0) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_set_rule(h, t, &rule) == NGW_E_INVALID_ARG);
                REQUIRE(ngw_tree_clear(h, t) == NGW_E_INVALID_ARG);
                tree_report(h, t);
            } else
                OK(ngw_key_table_destroy(h, table));
        }
        DESTROY(h);                                      // (the snapshot and the last tree still open)
    }
}

// ---------------------------------------------------------------- recipe
// Pogostick-v1's program (tests/test_recipe_heuristic_cpu.py, by item id: plank 2, pogo_stick 3, rubber 4, stick 5, tree_log 6, tree_tap 7); the tap
// counts on the map unless `map_items` is 0
ngw_recipe_program pogo_program(uint32_t map_items) {
    ngw_recipe_program p;
    memset(&p, 0, sizeof(p));
    p.goal_item = 3; p.n_rules = 6; p.map_items = map_items;
    auto rule = [&](int r, int out, int qty, int cost, int tool, std::initializer_list<int> in) {
        ngw_recipe_rule& u = p.rules[r];
        u.out_item = out; u.out_qty = qty; u.cost = cost; u.tool_item = tool;
        for (auto it = in.begin(); it != in.end(); it += 2) { u.in_item[u.n_in] = it[0]; u.in_qty[u.n_in++] = it[1]; }
    };
    rule(0, 3, 1, 8400, -1, {5, 4, 2, 2, 4, 1});
    rule(1, 4, 1, 50000, 7, {});
    rule(2, 7, 1, 7200, -1, {2, 5, 5, 1});
    rule(3, 5, 4, 2400, -1, {2, 2});
    rule(4, 2, 4, 1200, -1, {6, 1});
    rule(5, 6, 1, 3600, -1, {});
    return p;
}

void scenario_recipe() {
    const ngw_spec* sp = spec();
    const int64_t n = 130;
    ngw_handle* h = make(sp, n);
    const ngw_recipe_program with_map = pogo_program(1u << 7), without = pogo_program(0);
    for (int64_t cap : {(int64_t)1, (int64_t)64, (int64_t)65, (int64_t)130}) {
        ngw_snapshot* s = nullptr;
        OK(ngw_snapshot_create(h, cap, &s));
        for (const ngw_recipe_program* prog : {&with_map, &without})
            for (int64_t c : {(int64_t)0, (int64_t)1, cap}) {
                Arr<int32_t>* idx = iota_list((size_t)c);
                Arr<int32_t> out((size_t)c);
                OK(ngw_snapshot_recipe_costs(h, s, *idx, c, prog, out));
                OK(ngw_snapshot_recipe_costs(h, s, nullptr, c, prog, out));
                OK(ngw_snapshot_recipe_costs(h, nullptr, *idx, c, prog, out));     // the live envs (cap <= n of them)
                OK(ngw_snapshot_recipe_costs(h, nullptr, nullptr, c, prog, out));
                delete idx;
            }
        OK(ngw_snapshot_destroy(h, s));
    }
    // open-list searches with the term: one int32 per list entry, an allocation of its own
    int32_t costs[64];
    for (int i = 0; i < 64; i++) costs[i] = 1;
    Arr<int32_t> weights((size_t)sp->n_items, 1);
    ngw_snapshot* pool = nullptr; ngw_key_table* table = nullptr;
    OK(ngw_snapshot_create(h, 130, &pool));
    OK(ngw_key_table_create_valued(h, 1000, 0, &table));
    for (int64_t cap : {(int64_t)1, (int64_t)3, (int64_t)64, (int64_t)65})
        for (int32_t mode : {NGW_SEARCH_H_MIN, NGW_SEARCH_H_MAX}) {
            ngw_search_options o;
            memset(&o, 0, sizeof(o));
            o.capacity = cap; o.costs_host = costs; o.keep = mode == NGW_SEARCH_H_MIN ? 1 : (int32_t)cap; o.prune = 1;
            o.heuristic = mode; o.n_weights = sp->n_items; o.weights_host = weights;
            ngw_search* s = nullptr; ngw_search_arrays_open oarr;
            OK(ngw_search_create_open(h, pool, table, &o, &oarr, &s));
            if (cap == 3) arm("search_recipe_term");
            OK(ngw_search_set_recipe(h, s, mode == NGW_SEARCH_H_MIN ? &with_map : &without));
            OK(ngw_search_set_recipe(h, s, &with_map));                              // (again before the start: the same allocation serves)
            Arr<int32_t>* roots = iota_list((size_t)cap);
            int32_t cur = -1;
            OK(ngw_search_start(h, s, *roots, cap, &cur));                           // count == cap roots: the last entry of the term is written
            delete roots;
            OK(ngw_search_run(h, s, 2, &cur));
            search_reads(h, s, true);
            REQUIRE(ngw_search_set_recipe(h, s, &with_map) == NGW_E_INVALID_ARG);    // after ngw_search_start: refused
            if (cap != 65) OK(ngw_search_destroy(h, s));                             // (the last one, and its term, are ngw_destroy's to release)
        }
    DESTROY(h);
}

// ---------------------------------------------------------------- refusals
int g_refusals = 0;
void refused(int line, int rc, long long before) {
    if (rc != NGW_E_INVALID_ARG) die(line, "a call that must be refused did not return NGW_E_INVALID_ARG");
    if (!ngw_last_error() || !*ngw_last_error()) die(line, "a refusal without a message");
    if (fake_hip_live_total() != before) { fake_hip_report(); die(line, "a refused call left something in the ledger"); }
    g_refusals++;
}
#define REFUSED(expr) do { const long long _b = fake_hip_live_total(); refused(__LINE__, (expr), _b); } while (0)

void scenario_refusals() {
    const ngw_spec* sp = spec();
    ngw_handle* h = make(sp, 65);
    ngw_handle* other = make(sp, 1);
    int32_t costs[64] = {0};
    ngw_snapshot* pool = nullptr; ngw_key_table *plain = nullptr, *valued = nullptr, *foreign = nullptr; ngw_snapshot* foreign_pool = nullptr;
    OK(ngw_snapshot_create(h, 8, &pool));
    OK(ngw_key_table_create(h, 8, &plain));
    OK(ngw_key_table_create_valued(h, 8, 0, &valued));
    OK(ngw_key_table_create_valued(other, 8, 0, &foreign));
    OK(ngw_snapshot_create(other, 8, &foreign_pool));
    Arr<uint64_t> keys(8); Arr<int32_t> i32(64), j32(64), k32(64); Arr<uint8_t> u8(64), v8(64);
    ngw_key_table* t = nullptr; ngw_snapshot* s = nullptr; ngw_search* q = nullptr;
    ngw_search_arrays arr; ngw_search_arrays_open oarr;
    // tables
    REFUSED(ngw_key_table_create(h, 0, &t));
    REFUSED(ngw_key_table_create(h, (1ll << 29) + 1, &t));
    REFUSED(ngw_key_table_create(nullptr, 8, &t));
    REFUSED(ngw_key_table_create(h, 8, nullptr));
    REFUSED(ngw_key_table_create_valued(h, 8, (1ull << 62) + 1, &t));
    REFUSED(ngw_key_table_insert(h, foreign, keys, 8, i32, u8));
    REFUSED(ngw_key_table_insert(h, plain, nullptr, 8, i32, u8));
    REFUSED(ngw_key_table_insert(h, plain, keys, 8, nullptr, u8));
    REFUSED(ngw_key_table_insert(h, plain, keys, 8, i32, nullptr));
    REFUSED(ngw_key_table_insert(h, plain, keys, -1, i32, u8));
    REFUSED(ngw_key_table_lookup(h, plain, keys, -1, i32));
    REFUSED(ngw_key_table_lookup(h, foreign, keys, 8, i32));
    REFUSED(ngw_key_table_insert_min(h, plain, keys, i32, nullptr, 8, j32, u8, v8));
    REFUSED(ngw_key_table_insert_min(h, valued, keys, nullptr, nullptr, 8, j32, u8, v8));
    REFUSED(ngw_key_table_insert_min(h, valued, keys, i32, nullptr, 8, j32, u8, nullptr));
    REFUSED(ngw_key_table_insert_min(h, valued, keys, i32, nullptr, 0x80000000ll, j32, u8, v8));
    REFUSED(ngw_key_table_read(h, plain, i32, 8, j32, k32));
    REFUSED(ngw_key_table_read(h, valued, nullptr, 8, j32, k32));
    REFUSED(ngw_key_table_read(h, valued, i32, -1, j32, k32));
    REFUSED(ngw_key_table_trace(h, valued, i32, 8, -1, 4, j32, k32, k32));
    REFUSED(ngw_key_table_trace(h, valued, i32, 8, NGW_TRACE_MAX_STEPS + 1, 4, j32, k32, k32));
    REFUSED(ngw_key_table_trace(h, valued, i32, 8, 2, 4, nullptr, k32, k32));
    REFUSED(ngw_key_table_trace(h, valued, i32, 8, 2, 0, j32, k32, k32));
    REFUSED(ngw_key_table_trace(h, valued, i32, 8, 2, 0x7FFFFFFF, j32, k32, k32));
    REFUSED(ngw_key_table_trace(h, plain, i32, 8, 2, 4, j32, k32, k32));
    REFUSED(ngw_key_table_count(h, foreign, reinterpret_cast<int64_t*>(keys.get())));
    REFUSED(ngw_key_table_clear(h, foreign));
    REFUSED(ngw_key_table_destroy(h, foreign));
    // frontiers
    REFUSED(ngw_frontier_compact(h, u8, -1, 1, nullptr, 8, i32, j32, k32));
    REFUSED(ngw_frontier_compact(h, u8, (1ll << 24) + 1, 1, nullptr, 8, i32, j32, k32));
    REFUSED(ngw_frontier_compact(h, nullptr, 8, 1, nullptr, 8, i32, j32, k32));
    REFUSED(ngw_frontier_compact(h, u8, 8, 0, nullptr, 8, i32, j32, k32));
    REFUSED(ngw_frontier_compact(h, u8, 8, 1, nullptr, -1, i32, j32, k32));
    REFUSED(ngw_frontier_compact(h, u8, 8, 1, nullptr, 8, nullptr, j32, k32));
    REFUSED(ngw_frontier_compact(h, u8, 8, 1, nullptr, 8, i32, j32, nullptr));
    REFUSED(ngw_frontier_alloc(h, nullptr, i32, 8, 8, j32));
    REFUSED(ngw_frontier_alloc(h, k32, nullptr, 8, 8, j32));
    REFUSED(ngw_frontier_alloc(h, k32, i32, -1, 8, j32));
    REFUSED(ngw_frontier_alloc(h, k32, i32, 8, -1, j32));
    REFUSED(ngw_frontier_alloc(h, k32, i32, 8, 8, nullptr));
    // selections
    Arr<int32_t> taken(4), bound(4), count(2);
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 0, 8, j32, k32, nullptr, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 0, 8, j32, k32, taken, nullptr, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, nullptr));
    REFUSED(ngw_frontier_select(h, i32, nullptr, -1, 1, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, (1ll << 24) + 1, 1, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 0, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 3, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, nullptr, nullptr, 64, 1, 1, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 0, nullptr, 2, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, -1, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 2, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 0, -1, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 4, 1, nullptr, 3, 0, 8, j32, k32, taken, bound, count));
    REFUSED(ngw_frontier_select(h, i32, nullptr, 64, 1, 1, nullptr, 2, 0, 8, nullptr, k32, taken, bound, count));
    // searches
    REFUSED(ngw_search_create(h, nullptr, valued, 4, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 4, nullptr, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 4, costs, 0, -1, 0, nullptr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 4, costs, 0, -1, 0, &arr, nullptr));
    REFUSED(ngw_search_create(h, pool, plain, 4, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, foreign, 4, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, foreign_pool, valued, 4, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 0, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 9, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_create(h, pool, valued, 4, costs, 0, 5, 0, &arr, &q));
    ngw_search_options o;
    memset(&o, 0, sizeof(o));
    o.capacity = 4; o.costs_host = costs; o.keep = 0;
    REFUSED(ngw_search_create_open(h, pool, valued, &o, &oarr, &q));                 // keep < 1
    o.keep = 1; o.heuristic = 3;
    REFUSED(ngw_search_create_open(h, pool, valued, &o, &oarr, &q));                 // a heuristic mode other than the three
    o.heuristic = NGW_SEARCH_H_MIN; o.n_weights = sp->n_items; o.weights_host = nullptr;
    REFUSED(ngw_search_create_open(h, pool, valued, &o, &oarr, &q));                 // NULL weights
    Arr<int32_t> w((size_t)sp->n_items, 1);
    o.weights_host = w; o.n_weights = sp->n_items - 1;
    REFUSED(ngw_search_create_open(h, pool, valued, &o, &oarr, &q));                 // n_weights != n_items
    o.n_weights = sp->n_items; w[1] = -1;
    REFUSED(ngw_search_create_open(h, pool, valued, &o, &oarr, &q));                 // a negative weight
    REFUSED(ngw_search_create_open(h, pool, valued, nullptr, &oarr, &q));
    OK(ngw_search_create(h, pool, valued, 4, costs, 0, -1, 0, &arr, &q));
    REFUSED(ngw_search_start(h, q, i32, -1, nullptr));
    REFUSED(ngw_search_start(h, q, i32, 5, nullptr));
    REFUSED(ngw_search_start(h, q, nullptr, 2, nullptr));
    REFUSED(ngw_search_run(h, q, -1, nullptr));
    REFUSED(ngw_search_read(h, q, nullptr));
    REFUSED(ngw_search_read_open(h, q, reinterpret_cast<ngw_search_open_report*>(keys.get())));   // (a search without an open list: refused before `out` is touched)
    REFUSED(ngw_search_run(other, q, 1, nullptr));
    REFUSED(ngw_search_destroy(other, q));
    {   // tree-search runs: ngw_tree_create, ngw_tree_start, ngw_tree_set_rule and the staged calls' stage_args, one rule each
        ngw_tree* tr = nullptr;
        ngw_tree_options to;
        memset(&to, 0, sizeof(to));
        to.playouts = 4; to.steps = 3; to.fields = NGW_KEY_STATE; to.c = 1.0f;
        ngw_tree_options bad = to;
        REFUSED(ngw_tree_create(h, nullptr, &to, &tr));
        REFUSED(ngw_tree_create(h, plain, nullptr, &tr));
        REFUSED(ngw_tree_create(h, plain, &to, nullptr));
        REFUSED(ngw_tree_create(h, foreign, &to, &tr));
        bad.playouts = 0; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.steps = 0; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.playouts = 1ll << 31; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.playouts = 1 << 20; bad.steps = 1 << 12; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.fields = 0; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.fields = NGW_KEY_ALL + 1; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.c = 1.0f / 0.0f; REFUSED(ngw_tree_create(h, plain, &bad, &tr)); bad = to;
        bad.q_init = 0.0f / 0.0f; REFUSED(ngw_tree_create(h, plain, &bad, &tr));
        OK(ngw_tree_create(h, plain, &to, &tr));
        REFUSED(ngw_tree_start(h, tr, foreign_pool, i32, 2));
        REFUSED(ngw_tree_start(h, tr, pool, i32, -1));
        REFUSED(ngw_tree_start(h, tr, pool, i32, 5));
        REFUSED(ngw_tree_start(h, tr, pool, nullptr, 2));
        REFUSED(ngw_tree_start(other, tr, nullptr, i32, 2));
        REFUSED(ngw_tree_run(h, tr, -1, 0));
        ngw_tree_rule rule = {1, 65536, 0, 0};
        REFUSED(ngw_tree_set_rule(h, tr, nullptr));
        rule.spread = 0; REFUSED(ngw_tree_set_rule(h, tr, &rule));
        rule.spread = 65; REFUSED(ngw_tree_set_rule(h, tr, &rule)); rule.spread = 1;
        rule.discount_q16 = -1; REFUSED(ngw_tree_set_rule(h, tr, &rule));
        rule.discount_q16 = 65537; REFUSED(ngw_tree_set_rule(h, tr, &rule)); rule.discount_q16 = 65536;
        rule.rows16 = 3; REFUSED(ngw_tree_set_rule(h, tr, &rule));
        rule.rows16 = 2; rule.spread = 2; REFUSED(ngw_tree_set_rule(h, tr, &rule)); rule.rows16 = 0; rule.spread = 1;
        rule.reserved = 1; REFUSED(ngw_tree_set_rule(h, tr, &rule));
        REFUSED(ngw_tree_grow(h, tr, i32, j32, keys, keys, 4, -1, 1));               // stage_args: count, n_steps, stride
        REFUSED(ngw_tree_grow(h, tr, i32, j32, keys, keys, 8, 5, 1));
        REFUSED(ngw_tree_grow(h, tr, i32, j32, keys, keys, 4, 4, 0));
        REFUSED(ngw_tree_grow(h, tr, i32, j32, keys, keys, 4, 4, 4));
        REFUSED(ngw_tree_grow(h, tr, i32, j32, keys, keys, 3, 4, 1));
        REFUSED(ngw_tree_grow(h, tr, nullptr, j32, keys, keys, 4, 4, 1));
        REFUSED(ngw_tree_backup(h, tr, i32, j32, k32, i32, j32, 3, 4, 1, 0, nullptr));
        REFUSED(ngw_tree_backup(h, tr, i32, nullptr, k32, i32, j32, 4, 4, 1, 0, nullptr));
        REFUSED(ngw_tree_reweight(h, tr, i32, -1));
        REFUSED(ngw_tree_report(h, tr, nullptr));
        REFUSED(ngw_tree_arrays(h, tr, nullptr));
        REFUSED(ngw_tree_destroy(other, tr));
        OK(ngw_tree_destroy(h, tr));
    }
    {   // recipe programs: the rules of recipe_pack, one each (the call of no rows makes every check)
        const ngw_recipe_program good = pogo_program(1u << 7);
        const int32_t K = sp->n_items;
        auto refuse = [&](int line, const ngw_recipe_program& p) {
            const long long before = fake_hip_live_total();
            refused(line, ngw_snapshot_recipe_costs(h, nullptr, nullptr, 0, &p, i32), before);
        };
        OK(ngw_snapshot_recipe_costs(h, nullptr, nullptr, 0, &good, i32));
        REFUSED(ngw_snapshot_recipe_costs(h, nullptr, nullptr, 0, nullptr, i32));
        REFUSED(ngw_snapshot_recipe_costs(h, nullptr, nullptr, 0, &good, nullptr));
        REFUSED(ngw_snapshot_recipe_costs(h, foreign_pool, nullptr, 0, &good, i32));
        REFUSED(ngw_snapshot_recipe_costs(h, nullptr, nullptr, -1, &good, i32));
        REFUSED(ngw_snapshot_recipe_costs(h, nullptr, nullptr, 66, &good, i32));      // more rows than envs, without a list
        ngw_recipe_program p = good;
        p.n_rules = NGW_RECIPE_MAX_RULES + 1; refuse(__LINE__, p); p = good;
        p.goal_item = K; refuse(__LINE__, p); p = good;
        p.map_items = 1u << K; refuse(__LINE__, p); p = good;
        p.rules[1].out_item = -1; refuse(__LINE__, p); p = good;
        p.rules[1].out_item = 3; refuse(__LINE__, p); p = good;                        // two rules give item 3
        p.rules[1].out_qty = 0; refuse(__LINE__, p); p = good;
        p.rules[1].cost = -1; refuse(__LINE__, p); p = good;
        p.rules[1].n_in = NGW_RECIPE_MAX_INPUTS + 1; refuse(__LINE__, p); p = good;
        p.rules[0].in_item[0] = K; refuse(__LINE__, p); p = good;
        p.rules[0].in_qty[0] = 65536; refuse(__LINE__, p); p = good;
        p.map_items = 1u << 2; refuse(__LINE__, p); p = good;                          // plank: consumed by rule 0 and counted on the map
        p.rules[1].tool_item = -2; refuse(__LINE__, p); p = good;
        p.map_items = (1u << 0) | (1u << 1) | (1u << 3) | (1u << 7) | (1u << 8); refuse(__LINE__, p); p = good;   // five flagged items, none consumed
        p.rules[2].tool_item = 3; refuse(__LINE__, p); p = good;                       // a tool given by an EARLIER rule
        p.rules[5].in_item[0] = 2; p.rules[5].in_qty[0] = 1; p.rules[5].n_in = 1; refuse(__LINE__, p);   // an input given by an earlier rule
    }
    OK(ngw_snapshot_destroy(h, pool));                   // the search's pool closed: the refusal path
    REFUSED(ngw_search_run(h, q, 1, nullptr));
    REFUSED(ngw_search_start(h, q, nullptr, 0, nullptr));
    OK(ngw_search_destroy(h, q));
    REFUSED(ngw_snapshot_create(h, 0, &s));
    {   // maps whose two sets of 64 rows exceed the LDS of a CU: the second spec file (36 x 36); the search and the successor keys are refused
        REQUIRE(g_specs.size() >= 2 && spec(1)->map_size >= 36);
        ngw_handle* big = make(spec(1), 65);
        ngw_snapshot* bpool = nullptr; ngw_key_table* btable = nullptr;
        OK(ngw_snapshot_create(big, 8, &bpool));
        OK(ngw_key_table_create_valued(big, 8, 0, &btable));
        REFUSED(ngw_search_create(big, bpool, btable, 4, costs, 0, -1, 0, &arr, &q));
        o.keep = 1; o.heuristic = NGW_SEARCH_H_NONE;
        REFUSED(ngw_search_create_open(big, bpool, btable, &o, &oarr, &q));
        REFUSED(ngw_successor_keys(big, bpool, nullptr, 4, NGW_KEY_STATE, keys, nullptr, nullptr, nullptr));
        // a tree's guided playout keeps ONE set of maps: 36 x 36 fits, and the tree is made
        ngw_tree* btree = nullptr;
        ngw_tree_options to;
        memset(&to, 0, sizeof(to));
        to.playouts = 4; to.steps = 3; to.fields = NGW_KEY_STATE; to.c = 1.0f;
        OK(ngw_tree_create(big, btable, &to, &btree));
        OK(ngw_tree_destroy(big, btree));
        OK(ngw_destroy(big));
    }
    {   // maps beyond the guided playout's limit: the third spec file (48 x 48).  ngw_tree_create's call of no pairs refuses it AFTER the slab exists:
        // the error path has to release it
        REQUIRE(g_specs.size() >= 3 && spec(2)->map_size >= 48);
        ngw_handle* huge = make(spec(2), 65);
        ngw_key_table* htable = nullptr; ngw_tree* htree = nullptr;
        OK(ngw_key_table_create(huge, 8, &htable));
        ngw_tree_options to;
        memset(&to, 0, sizeof(to));
        to.playouts = 4; to.steps = 3; to.fields = NGW_KEY_STATE; to.c = 1.0f;
        REFUSED(ngw_tree_create(huge, htable, &to, &htree));
        REQUIRE(htree == nullptr && strstr(ngw_last_error(), "map_size") != nullptr);
        OK(ngw_destroy(huge));
    }
    REFUSED(ngw_snapshot_destroy(h, foreign_pool));
    (void)t;
    REQUIRE(g_refusals > 80);
    OK(ngw_destroy(other));                              // (its table and snapshot still open)
    DESTROY(h);                                          // (likewise; the ledger counts both handles, so it is read after the second)
}

// ---------------------------------------------------------------- the ledger's own check: an allocation nobody frees must end the program non-zero
void scenario_leak_selfcheck() {
    ngw_handle* h = make(spec(), 1);
    void* lost = nullptr;
    REQUIRE(hipMalloc(&lost, 24) == hipSuccess);
    DESTROY(h);
}

}  // namespace

int main(int argc, char** argv) {
    setenv("NGW_SOLO", "0", 1);                          // the one-env resident loop is out of scope
    if (argc < 3) { fprintf(stderr, "usage: %s <scenario> <spec file> [<spec file> ...] [short=<allocation>]\n", argv[0]); return 2; }
    g_scenario = argv[1];
    for (int i = 2; i < argc; i++) {
        if (!strncmp(argv[i], "short=", 6)) { g_short = argv[i] + 6; continue; }
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "hostcheck: cannot open %s\n", argv[i]); return 2; }
        std::vector<uint8_t> bytes((size_t)ngw_spec_size() + 1);
        const size_t got = fread(bytes.data(), 1, bytes.size(), f);
        fclose(f);
        if (got != (size_t)ngw_spec_size()) { fprintf(stderr, "hostcheck: %s holds %zu bytes, ngw_spec_size() is %d\n", argv[i], got, ngw_spec_size()); return 2; }
        bytes.resize(got);
        g_specs.push_back(bytes);
    }
    if (g_specs.empty()) { fprintf(stderr, "hostcheck: no spec file\n"); return 2; }
    if (!g_short.empty() && !fake_hip_short_bytes()) { fprintf(stderr, "hostcheck: short= needs the -DFAKE_HIP_SHORT build\n"); return 2; }
    if (!g_short.empty()) fake_hip_short_only(-1);       // nothing is short until arm() picks the named allocation ("none": the short build's clean run)
    const std::string s = g_scenario;
    if (s == "handle") scenario_handle();
    else if (s == "host_step") scenario_host_step();
    else if (s == "snapshot") scenario_snapshot();
    else if (s == "table") scenario_table();
    else if (s == "frontier") scenario_frontier();
    else if (s == "search") scenario_search();
    else if (s == "tree") scenario_tree();
    else if (s == "recipe") scenario_recipe();
    else if (s == "refusals") scenario_refusals();
    else if (s == "leak_selfcheck") scenario_leak_selfcheck();
    else { fprintf(stderr, "hostcheck: unknown scenario '%s'\n", g_scenario); return 2; }
    if (!g_short.empty() && g_short != "none" && !g_short_armed) { fprintf(stderr, "hostcheck: scenario '%s' never makes the allocation '%s'\n", g_scenario, g_short.c_str()); return 3; }
    if (fake_hip_live_total() != 0) { fake_hip_report(); die(__LINE__, "the ledger is not empty at the end of the scenario"); }
    printf("hostcheck: scenario '%s' passed\n", g_scenario);
    return 0;
}
