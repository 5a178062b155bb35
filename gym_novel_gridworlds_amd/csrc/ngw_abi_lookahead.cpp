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

// [A][n] rows as they arrive from the device -> the caller's env-major [n][A]
template <typename T>
void to_env_major(const std::vector<T>& rows, T* out, int64_t n, int A) {
    for (int a = 0; a < A; a++) {
        const T* src = rows.data() + (size_t)a * (size_t)n;
        for (int64_t i = 0; i < n; i++) out[(size_t)i * (size_t)A + (size_t)a] = src[i];
    }
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
    const int A = h->spec.n_actions;
    const size_t n = (size_t)h->n, cells = n * (size_t)A;
    std::vector<int32_t> r(reward ? cells : 0);
    std::vector<uint8_t> d(done ? cells : 0);
    std::vector<uint32_t> w(info ? cells : 0);
    // row a of the device table is n_pad long: one strided copy per array brings the n live columns of every row across
    if (reward) HIP_TRY(hipMemcpy2DAsync(r.data(), n * 4, h->look_reward, (size_t)h->n_pad * 4, n * 4, (size_t)A, hipMemcpyDefault, h->stream));
    if (done) HIP_TRY(hipMemcpy2DAsync(d.data(), n, h->look_done, (size_t)h->n_pad, n, (size_t)A, hipMemcpyDefault, h->stream));
    if (info) HIP_TRY(hipMemcpy2DAsync(w.data(), n * 4, h->look_info, (size_t)h->n_pad * 4, n * 4, (size_t)A, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (reward) to_env_major(r, reward, h->n, A);
    if (done) to_env_major(d, done, h->n, A);
    if (info) to_env_major(w, info, h->n, A);
    return NGW_OK;
}

int ngw_lookahead_device_ptrs(ngw_handle* h, void** reward, void** done, void** info, int64_t* env_stride, int64_t* action_stride) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    HIP_TRY(hipSetDevice(h->device));
    if (!h->look_info) {
        if (h->solo_running) { if (int rc = solo_stop(h)) return rc; }   // (the allocation zero-fills on the handle's stream)
        if (int rc = alloc_table(h)) return rc;
    }
    if (reward) *reward = h->look_reward;
    if (done) *done = h->look_done;
    if (info) *info = h->look_info;
    if (env_stride) *env_stride = 1;
    if (action_stride) *action_stride = h->n_pad;
    return NGW_OK;
}

}  // extern "C"
