// ngw_abi_lookahead.cpp - one-step lookahead tables (see ngw_host.h): the lookahead kernel (ngw_lookahead.inc) on demand, whether the
// handle's table describes its current state, and the one-env handle's answer from the resident loop's speculated records.
#include "ngw_host.h"

using namespace ngwh;

namespace {

// the three arrays, action-major [n_actions][n_pad] (zero-filled on the handle's stream); no-op once allocated
int alloc_table(ngw_handle* h) {
    if (h->look_info) return NGW_OK;
    const size_t cells = (size_t)h->spec.n_actions * (size_t)h->n_pad;
    if (int rc = dev_alloc(h, &h->look_reward, cells)) return rc;
    if (int rc = dev_alloc(h, &h->look_done, cells)) return rc;
    return dev_alloc(h, &h->look_info, cells);
}

// The table is current when nothing has written the state since it was computed (state_written) and it was computed under the autoreset
// setting the next step would run under (ngw_set_autoreset changes what a step reports, not the state).
bool table_current(const ngw_handle* h) { return h->look_fresh && h->look_autoreset == h->autoreset && h->look_horizon == h->horizon; }

int run_table(ngw_handle* h) {
    if (int rc = alloc_table(h)) return rc;
    HIP_TRY(ngw_lookahead_launch(h->dspec, &h->b, h->n, h->n_pad, h->proto.S, h->proto.K, h->ext, h->autoreset, h->horizon, h->look_reward,
                                 h->look_done, h->look_info, (unsigned)(h->n_pad / NGW_EPB), h->stream));
    h->look_fresh = true; h->look_autoreset = h->autoreset; h->look_horizon = h->horizon;
    return NGW_OK;
}

// The one-env loop speculates every action from the committed state: record a holds exactly what step(a) would report (reference semantics:
// the records know no horizon, so a handle whose autoreset was turned on while the loop runs is not answered from them).  False when the
// records do not describe what the next step would report: the caller runs the kernel instead.
bool solo_table(ngw_handle* h, int32_t* reward, uint8_t* done, uint32_t* info) {
    if (h->autoreset || !solo_records_ready(h)) return false;
    const NgwSolo& p = h->solo_proto;
    for (int a = 0; a < p.A; a++) {
        const uint32_t* rec = h->solo_out + NGW_SOLO_REC0 + (size_t)a * (size_t)p.rec_dw;
        if (reward) reward[a] = (int32_t)rec[0];
        if (done) done[a] = (uint8_t)(rec[2] & 1u);
        if (info) info[a] = rec[1];
    }
    return true;
}

}  // namespace

extern "C" {

int ngw_lookahead(ngw_handle* h) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (int rc = enter(h)) return rc;
    if (!table_current(h)) { if (int rc = run_table(h)) return rc; }
    return NGW_OK;
}

int ngw_get_lookahead(ngw_handle* h, int32_t* reward, uint8_t* done, uint32_t* info) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (h->solo_running && solo_table(h, reward, done, info)) return NGW_OK;    // (the one-env loop keeps running: no relaunch per query)
    if (int rc = ngw_lookahead(h)) return rc;
    return fetch_env_major(h, h->spec.n_actions, {{h->look_reward, reward, 4}, {h->look_done, done, 1}, {h->look_info, info, 4}});
}

int ngw_lookahead_device_ptrs(ngw_handle* h, void** reward, void** done, void** info, int64_t* env_stride, int64_t* action_stride) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (int rc = enter_to_allocate(h, h->look_info != nullptr)) return rc;
    if (int rc = alloc_table(h)) return rc;
    if (reward) *reward = h->look_reward;
    if (done) *done = h->look_done;
    if (info) *info = h->look_info;
    if (env_stride) *env_stride = 1;
    if (action_stride) *action_stride = h->n_pad;
    return NGW_OK;
}

}  // extern "C"
