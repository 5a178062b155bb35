// ngw_unit_recipe.hip — the recipe heuristic (ngw_recipe.inc): crafting-cost lower bounds of saved slots and live envs.
#include "ngw_common.inc"
#include "ngw_recipe.inc"

// x->count costs of rows of x->src through the index list; one wave per 64 entries.  The program is checked here as far as the kernel's addressing
// depends on it (the host unit has refused everything else): rule and slot numbers in range, items below K.
extern "C" hipError_t ngw_recipe_launch(const NgwRecipe* x, hipStream_t stream) {
    const int64_t blocks = blocks_for(x->count);
    if (x->count <= 0 || blocks > 0x7FFFFFFFll || x->rows < 1 || x->S2 < 9 || x->S2 > NGW_MAX_MAP_SIZE * NGW_MAX_MAP_SIZE || x->K < 1 || x->K > NGW_MAX_ITEMS ||
        !x->flags || !x->src.map || !x->src.inv || !x->out)
        return hipErrorInvalidValue;
    const NgwRecipeProg& p = x->prog;
    if (p.n_rules < 0 || p.n_rules > NGW_RECIPE_RULES || p.goal_rule < -1 || p.goal_rule >= p.n_rules || p.n_map < 0 || p.n_map > 4) return hipErrorInvalidValue;
    for (int i = 0; i < p.n_map; i++)
        if (p.map_item[i] >= x->K) return hipErrorInvalidValue;
    for (int r = 0; r < p.n_rules; r++) {
        const NgwRecipeRule& u = p.rule[r];
        if (u.cost < 0 || u.out_qty < 1 || u.out_item >= x->K || u.n_in > 4 || u.map_slot < -1 || u.map_slot >= p.n_map || u.tool_rule < -1 ||
            (u.tool_rule >= 0 && (u.tool_rule <= r || u.tool_rule >= p.n_rules)))
            return hipErrorInvalidValue;
        for (int i = 0; i < u.n_in; i++)
            if (u.in_rule[i] < -1 || (u.in_rule[i] >= 0 && (u.in_rule[i] <= r || u.in_rule[i] >= p.n_rules)) || u.in_qty[i] < 1) return hipErrorInvalidValue;
    }
    const dim3 grid((unsigned)blocks), block(NGW_EPB);
    return with_row_piece(x->S2, [&](auto V) { return launch_kernel<ngw_recipe_kernel<decltype(V)::value>>(grid, block, 0, stream, *x); });
}
