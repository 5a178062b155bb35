// ngw_unit_plans.hip — plan evaluation (ngw_plans.inc).
#include "ngw_common.inc"
#include "ngw_plans.inc"

// a = the handle's rollout layout with a.actions = the plans, a.t0 = their env stride, a.n_steps, a.autoreset, a.horizon;
// grid = n_plans * n_pad / NGW_EPB work-groups
extern "C" hipError_t ngw_plans_launch(const NgwDevSpec* dspec, const NgwLaunch* a, const NgwPlan* pa, int map_mode, int ext, size_t lds_bytes, hipStream_t stream) {
    const uint64_t grid = (uint64_t)pa->n_plans * (uint64_t)(a->n_pad / NGW_EPB);
    if (a->n <= 0 || a->n_pad < a->n || a->n_pad % NGW_EPB || pa->n_plans < 1 || a->n_steps < 1 || a->t0 < a->n || grid * NGW_EPB > 0xFFFFFFFFull ||
        a->S < 3 || a->S > NGW_MAX_MAP_SIZE || a->K < 1 || a->K > NGW_MAX_ITEMS || !a->actions || !pa->ret || !pa->length || !pa->ended || !pa->info)
        return hipErrorInvalidValue;
    return with_map_mode(map_mode, [&](auto MM) {
        return with_flag(ext != 0, [&](auto E) {
            return launch_kernel<ngw_plans_lean<decltype(MM)::value, decltype(E)::value>>(dim3((unsigned)grid), dim3(NGW_EPB), lds_bytes, stream, dspec, *a, *pa);
        });
    });
}
