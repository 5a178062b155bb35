// ngw_abi_plans.cpp - plan evaluation (see ngw_host.h): n_plans candidate action sequences per env scored from the handle's current state by
// one launch of the plan kernel (ngw_plans.inc), and the result buffers.  The call commits nothing, so it neither calls state_written() nor
// touches anything the handle derives from its state; it counts no steps against the prepared-episode cadence either (no reset runs).
#include "ngw_host.h"

using namespace ngwh;

namespace {

// the four arrays, plan-major [n_plans][n_pad] (zero-filled on the handle's stream); regrown when a call brings more plans than any before
int alloc_results(ngw_handle* h, int32_t n_plans) {
    if (h->plan_info && n_plans <= h->plan_cap) return NGW_OK;
    if (h->plan_info) {
        HIP_TRY(hipStreamSynchronize(h->stream));                                  // (an evaluation may still be writing the old ones)
        dev_free(h, h->plan_ret); dev_free(h, h->plan_len); dev_free(h, h->plan_ended); dev_free(h, h->plan_info);
        h->plan_ret = nullptr; h->plan_len = nullptr; h->plan_ended = nullptr; h->plan_info = nullptr;
        h->plan_cap = 0; h->plan_n = 0;
    } else {
        const char* order = getenv("NGW_PLAN_ORDER");
        h->plan_major = order && !strcmp(order, "plan");
    }
    const size_t cells = (size_t)n_plans * (size_t)h->n_pad;
    if (int rc = dev_alloc(h, &h->plan_ret, cells)) return rc;
    if (int rc = dev_alloc(h, &h->plan_len, cells)) return rc;
    if (int rc = dev_alloc(h, &h->plan_ended, cells)) return rc;
    if (int rc = dev_alloc(h, &h->plan_info, cells)) return rc;
    h->plan_cap = n_plans;
    return NGW_OK;
}

}  // namespace

extern "C" {

int ngw_plan_eval(ngw_handle* h, const int32_t* plans_dev, int64_t env_stride, int32_t n_plans, int32_t n_steps) {
    if (!h || !plans_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (n_plans < 1) return fail(NGW_E_INVALID_ARG, "n_plans must be >= 1");
    if (n_steps < 1) return fail(NGW_E_INVALID_ARG, "n_steps must be >= 1");
    if (env_stride < h->n) return fail(NGW_E_INVALID_ARG, "env_stride %lld is smaller than n_envs", (long long)env_stride);
    if ((uint64_t)n_plans * (uint64_t)h->n_pad > 0xFFFFFFFFull)
        return fail(NGW_E_INVALID_ARG, "n_plans %d x %lld envs: the launch grid does not fit 32 bits", n_plans, (long long)h->n_pad);
    if (!h->general_ok)
        return fail(NGW_E_INVALID_ARG, "map_size %d: this call keeps a wavefront's 64 maps in LDS (ngw_plan_eval, as the fused rollouts) "
                                       "and they need more than 160 KiB; per-launch steps and resets are available", h->proto.S);
    if (int rc = enter(h)) return rc;
    if (int rc = alloc_results(h, n_plans)) return rc;
    NgwLaunch a = h->proto;
    a.b = h->b;
    a.mode = NGW_MODE_ROLLOUT_ACT;
    a.n_steps = n_steps;
    a.actions = plans_dev;
    a.t0 = env_stride;
    a.autoreset = h->autoreset;
    a.horizon = h->horizon;
    NgwPlan pa{};
    pa.ret = h->plan_ret; pa.length = h->plan_len; pa.ended = h->plan_ended; pa.info = h->plan_info;
    pa.n_plans = n_plans; pa.plan_major = h->plan_major;
    HIP_TRY(ngw_plans_launch(h->dspec, &a, &pa, h->map_mode, h->ext, h->lds_bytes, h->stream));
    h->plan_n = n_plans;
    return NGW_OK;
}

int ngw_get_plan_eval(ngw_handle* h, int32_t* ret, int32_t* length, uint8_t* ended, uint32_t* info) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (!h->plan_n) return fail(NGW_E_INVALID_ARG, "ngw_get_plan_eval before ngw_plan_eval");
    if (int rc = enter(h)) return rc;
    return fetch_env_major(h, h->plan_n, {{h->plan_ret, ret, 4}, {h->plan_len, length, 4}, {h->plan_ended, ended, 1}, {h->plan_info, info, 4}});
}

int ngw_plan_eval_device_ptrs(ngw_handle* h, void** ret, void** length, void** ended, void** info, int64_t* env_stride, int64_t* plan_stride) {
    if (!h) return fail(NGW_E_INVALID_ARG, "handle is NULL");
    if (!h->plan_n) return fail(NGW_E_INVALID_ARG, "ngw_plan_eval_device_ptrs before ngw_plan_eval");
    if (int rc = enter(h)) return rc;
    if (int rc = alloc_results(h, h->plan_n)) return rc;                           // (they exist since the evaluation: nothing is allocated here)
    if (ret) *ret = h->plan_ret;
    if (length) *length = h->plan_len;
    if (ended) *ended = h->plan_ended;
    if (info) *info = h->plan_info;
    if (env_stride) *env_stride = 1;
    if (plan_stride) *plan_stride = h->n_pad;
    return NGW_OK;
}

}  // extern "C"
