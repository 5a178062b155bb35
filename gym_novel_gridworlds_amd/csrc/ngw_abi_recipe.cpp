// ngw_abi_recipe.cpp - the recipe heuristic's host side (see ngw_host.h): the checks of a caller's program, its packed form, the one launch of
// ngw_recipe.inc, and ngw_snapshot_recipe_costs; the search's term (ngw_search_set_recipe, ngw_abi_search.cpp) goes through the first two.  Nothing
// here commits anything: no state_written(), no derived-state flag.
#include "ngw_host.h"

using namespace ngwh;

namespace ngwh {

// The rules of include/ngw.h, one message each; -> the program as the kernel takes it: items resolved to rule numbers, flagged items to count slots.
int recipe_pack(const ngw_handle* h, const ngw_recipe_program* in, NgwRecipeProg* out) {
    const int32_t K = h->proto.K;
    memset(out, 0, sizeof(*out));
    if (in->n_rules < 0 || in->n_rules > NGW_RECIPE_MAX_RULES) return fail(NGW_E_INVALID_ARG, "recipe program: %d rules (at most %d)", (int)in->n_rules, NGW_RECIPE_MAX_RULES);
    if (in->goal_item < 0 || in->goal_item >= K) return fail(NGW_E_INVALID_ARG, "recipe program: goal item %d outside [0, %d)", (int)in->goal_item, (int)K);
    if (K < 32 && (in->map_items >> K)) return fail(NGW_E_INVALID_ARG, "recipe program: map_items 0x%x flags an item outside [0, %d)", (unsigned)in->map_items, (int)K);
    int rule_of[NGW_MAX_ITEMS];
    for (int k = 0; k < NGW_MAX_ITEMS; k++) rule_of[k] = -1;
    for (int r = 0; r < in->n_rules; r++) {
        const ngw_recipe_rule& u = in->rules[r];
        if (u.out_item < 0 || u.out_item >= K) return fail(NGW_E_INVALID_ARG, "recipe rule %d: out_item %d outside [0, %d)", r, (int)u.out_item, (int)K);
        if (rule_of[u.out_item] >= 0) return fail(NGW_E_INVALID_ARG, "recipe rules %d and %d both give item %d", rule_of[u.out_item], r, (int)u.out_item);
        rule_of[u.out_item] = r;
        if (u.out_qty < 1 || u.out_qty > 65535) return fail(NGW_E_INVALID_ARG, "recipe rule %d: out_qty %d outside [1, 65535]", r, (int)u.out_qty);
        if (u.cost < 0 || u.cost == NGW_VALUE_NONE) return fail(NGW_E_INVALID_ARG, "recipe rule %d: cost %d outside [0, 2^31 - 1)", r, (int)u.cost);
        if (u.n_in < 0 || u.n_in > NGW_RECIPE_MAX_INPUTS) return fail(NGW_E_INVALID_ARG, "recipe rule %d: %d inputs (at most %d)", r, (int)u.n_in, NGW_RECIPE_MAX_INPUTS);
        for (int i = 0; i < u.n_in; i++) {
            if (u.in_item[i] < 0 || u.in_item[i] >= K) return fail(NGW_E_INVALID_ARG, "recipe rule %d: input item %d outside [0, %d)", r, (int)u.in_item[i], (int)K);
            if (u.in_qty[i] < 1 || u.in_qty[i] > 65535) return fail(NGW_E_INVALID_ARG, "recipe rule %d: input quantity %d outside [1, 65535]", r, (int)u.in_qty[i]);
            if (in->map_items >> u.in_item[i] & 1u)
                return fail(NGW_E_INVALID_ARG, "recipe rule %d consumes item %d, which map_items counts on the map", r, (int)u.in_item[i]);
        }
        if (u.tool_item < -1 || u.tool_item >= K) return fail(NGW_E_INVALID_ARG, "recipe rule %d: tool item %d outside [-1, %d)", r, (int)u.tool_item, (int)K);
    }
    int slot_of[NGW_MAX_ITEMS];
    for (int k = 0; k < K; k++) {
        slot_of[k] = -1;
        if (in->map_items >> k & 1u) {
            if (out->n_map == NGW_RECIPE_MAX_MAP_ITEMS) return fail(NGW_E_INVALID_ARG, "recipe program: map_items 0x%x flags more than %d items", (unsigned)in->map_items, NGW_RECIPE_MAX_MAP_ITEMS);
            slot_of[k] = out->n_map;
            out->map_item[out->n_map++] = (uint8_t)k;
        }
    }
    out->n_rules = in->n_rules;
    out->goal_rule = rule_of[in->goal_item];
    for (int r = 0; r < in->n_rules; r++) {
        const ngw_recipe_rule& u = in->rules[r];
        NgwRecipeRule& p = out->rule[r];
        p.cost = u.cost; p.out_qty = (uint16_t)u.out_qty; p.out_item = (uint8_t)u.out_item; p.n_in = (uint8_t)u.n_in;
        p.map_slot = (int8_t)slot_of[u.out_item];
        p.tool_rule = (int8_t)(u.tool_item >= 0 ? rule_of[u.tool_item] : -1);
        if (p.tool_rule >= 0 && p.tool_rule <= r)
            return fail(NGW_E_INVALID_ARG, "recipe rule %d: its tool, item %d, is given by rule %d - consumers come first", r, (int)u.tool_item, (int)p.tool_rule);
        for (int i = 0; i < NGW_RECIPE_MAX_INPUTS; i++) {
            p.in_rule[i] = (int8_t)(i < u.n_in ? rule_of[u.in_item[i]] : -1);
            p.in_qty[i] = (uint16_t)(i < u.n_in ? u.in_qty[i] : 0);
            if (p.in_rule[i] >= 0 && p.in_rule[i] <= r)
                return fail(NGW_E_INVALID_ARG, "recipe rule %d: its input, item %d, is given by rule %d - consumers come first", r, (int)u.in_item[i], (int)p.in_rule[i]);
        }
    }
    return NGW_OK;
}

int recipe_run(ngw_handle* h, const NgwSnapRows& src, int64_t rows, const int32_t* idx_dev, int64_t count, const NgwRecipeProg& prog, int32_t* out_dev) {
    NgwRecipe x{};
    x.src = src; x.idx = idx_dev; x.flags = h->b.flags; x.out = out_dev;
    x.count = count; x.rows = (int32_t)rows; x.S2 = h->proto.S2; x.K = h->proto.K; x.prog = prog;
    HIP_TRY(ngw_recipe_launch(&x, h->stream));
    return NGW_OK;
}

}  // namespace ngwh

extern "C" {

int ngw_snapshot_recipe_costs(ngw_handle* h, ngw_snapshot* s, const int32_t* idx_dev, int64_t count, const ngw_recipe_program* program, int32_t* out_dev) {
    if (!h || !program || !out_dev) return fail(NGW_E_INVALID_ARG, "NULL argument");
    if (s && !is_open(h->snaps, s)) return fail(NGW_E_INVALID_ARG, "not an open snapshot of this handle");
    const Source from = source_of(h, s);
    if (count < 0 || count > 0x7FFFFFFFll * NGW_EPB) return fail(NGW_E_INVALID_ARG, "recipe costs of %lld rows", (long long)count);
    if (!idx_dev && count > from.rows) return fail(NGW_E_INVALID_ARG, "recipe costs of %lld rows from %lld %s", (long long)count, (long long)from.rows, from.unit);
    if (int rc = enter(h)) return rc;                 // (s == NULL: the one-env loop has ended, HBM holds the env's state)
    NgwRecipeProg prog;
    if (int rc = recipe_pack(h, program, &prog)) return rc;
    if (count == 0) return NGW_OK;
    return recipe_run(h, from.r, from.rows, idx_dev, count, prog, out_dev);
}

}  // extern "C"
