// ngw_abi_mask.cpp - action masks (see ngw_host.h): the standalone mask kernel (ngw_mask.inc) behind a step or on demand, whether the handle's
// mask words describe its current state, and the one-env handle's answer from the resident loop's speculated records.
#include "ngw_host.h"

using namespace ngwh;

namespace ngwh {

int alloc_act_mask(ngw_handle* h) {
    if (h->act_mask) return NGW_OK;
    uint64_t* p = nullptr;
    if (int rc = dev_alloc(h, &p, (size_t)h->n_pad)) return rc;
    HIP_TRY(hipMemcpyAsync(&h->dspec->amask, &p, sizeof(p), hipMemcpyDefault, h->stream));   // (the fused step kernels store there)
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->act_mask = p;
    return NGW_OK;
}

int launch_act_mask(ngw_handle* h) {
    if (int rc = alloc_act_mask(h)) return rc;
    HIP_TRY(ngw_mask_launch(h->dspec, &h->b, h->n, h->proto.S, h->proto.K, h->ext, h->act_mask, (unsigned)(h->n_pad / NGW_EPB), h->stream));
    h->act_mask_fresh = true;
    return NGW_OK;
}

// The one-env loop speculates every action from the committed state into records.  Returns false when the records do not belong to the
// host's state (the loop ended before it took the last command): the caller stops the loop and runs a kernel instead.  Waits for the
// records like solo_step does, never stops the loop.
bool solo_records_ready(ngw_handle* h) {
    volatile uint32_t* o = h->solo_out;
    for (uint64_t spin = 0;; spin++) {
        if (o[0] == h->solo_seq) break;
        if (o[1]) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if (o[0] == h->solo_seq) break;
            return false;
        }
        if (spin > (1ull << 26)) return false;
        cpu_pause();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return true;
}

}  // namespace ngwh

namespace {

// bit 0 of record a's info word is exactly `result` of step(a)
bool solo_mask(ngw_handle* h, uint64_t* out) {
    if (!solo_records_ready(h)) return false;
    const NgwSolo& p = h->solo_proto;
    uint64_t m = 0;
    for (int a = 0; a < p.A; a++) m |= (uint64_t)(h->solo_out[NGW_SOLO_REC0 + (size_t)a * (size_t)p.rec_dw + 1] & 1u) << a;
    out[0] = m;
    return true;
}

}  // namespace

extern "C" {

int ngw_set_action_mask(ngw_handle* h, int enable) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (int rc = enter(h)) return rc;
    if (enable) { if (int rc = alloc_act_mask(h)) return rc; }
    h->act_mask_on = enable != 0;
    return NGW_OK;
}

int ngw_action_mask(ngw_handle* h) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (int rc = enter(h)) return rc;
    if (!h->act_mask_fresh) { if (int rc = launch_act_mask(h)) return rc; }
    return NGW_OK;
}

int ngw_get_action_mask(ngw_handle* h, uint64_t* out_host) {
    if (!h || !out_host) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (h->solo_running && solo_mask(h, out_host)) return NGW_OK;    // (the one-env loop keeps running: no relaunch per step)
    if (int rc = ngw_action_mask(h)) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, h->act_mask, (size_t)h->n * sizeof(uint64_t), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return NGW_OK;
}

int ngw_action_mask_device_ptr(ngw_handle* h, void** out) {
    if (!h || !out) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (int rc = enter_to_allocate(h, h->act_mask != nullptr)) return rc;
    if (int rc = alloc_act_mask(h)) return rc;
    *out = h->act_mask;
    return NGW_OK;
}

}  // extern "C"
