"""Expected action masks from the unmodified CPU oracle: for every action, step a copy of the state and read `result`.  Nothing here
comes from the HIP path (tests/test_action_masks*.py compare the device's masks with these)."""
import numpy as np

from oracle.ngw_oracle import Oracle, State


def state_from(spec, map_, loc, facing, inv, sel, step_count=None):
    """An oracle State of n envs from row arrays (map [n, S*S] or [n, S, S])."""
    cs = spec.compile()
    n = len(loc)
    st = State(n, cs.map_size, cs.n_items)
    st.map[...] = np.asarray(map_).reshape(n, -1)
    st.loc[...], st.facing[...], st.inv[...], st.selected[...] = loc, facing, inv, sel
    if step_count is not None:
        st.step_count[...] = step_count
    return st


def oracle_mask_words(spec, st):
    """uint64 [n]: bit a = the oracle's `result` of step(a) from each env's state in `st` (autoreset off: result is the step's own)."""
    cs = spec.compile()
    o = Oracle(cs, st.n)
    words = np.zeros(st.n, np.uint64)
    for a in range(cs.n_actions):
        o.st = st.copy()
        o.step(np.full(st.n, a, np.int32))
        words |= (np.asarray(o.result).astype(np.uint64) & np.uint64(1)) << np.uint64(a)
    return words


def oracle_masks(spec, st):
    from gym_novel_gridworlds_amd.vec_env import unpack_action_masks
    return unpack_action_masks(oracle_mask_words(spec, st), spec.compile().n_actions)
