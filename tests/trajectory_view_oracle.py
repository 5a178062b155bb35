"""Expected AgentMap views of a trajectory (observe='agent_view') from the unmodified CPU oracle: trajectory_oracle.oracle_traj replays the actions and
hands back the row after every executed step, and slot_observe_oracle.expect_view - the oracle's agent_view on a host copy of rows - gives the
window, the facing id and the inventory of the parents (block 0) and of every visited row (block t + 1); zeros for every step a pair did not
execute.  Nothing here uses the device's own step or view code (tests/test_trajectory_views*.py compare the HIP path with these)."""
import functools

import numpy as np

import expand_oracle as XO
import path_key_oracle as KO
import slot_observe_oracle as OO
import slot_rollout_oracle as RO
import trajectory_oracle as TO

FIELDS = ('agent_map', 'agent_facing_id', 'inventory_items_quantity')


def expect_views(spec, rows, parents, e, view_size):
    """e: oracle_traj's dict for `parents` of `rows` -> {'agent_map' int8 [T + 1, count, W, W], 'agent_facing_id' int32 [T + 1, count],
    'inventory_items_quantity' int32 [T + 1, count, K]}."""
    steps, count = e['rewards'].shape
    length = e['reports']['length']
    parent_rows = RO._rows_of(XO.rows_state(spec, rows, np.asarray(parents, np.int64)))
    first = OO.expect_view(parent_rows, np.arange(count), view_size)
    out = {k: np.zeros((steps + 1,) + v.shape, v.dtype) for k, v in first.items()}
    for k in first:
        out[k][0] = first[k]
    for t in range(steps):
        ran = np.nonzero(length > t)[0]
        if not ran.size:
            break
        after = OO.expect_view(TO._stack([e['states'][(t, int(j))] for j in ran]), np.arange(len(ran)), view_size)
        for k in first:
            out[k][t + 1, ran] = after[k]
    return out


def assert_views(got, exp, where):
    """Every field of a result's dict `obs` equals the oracle's, bit for bit: keys, dtypes, shapes, values."""
    got = OO.host(got)
    assert isinstance(got, dict) and sorted(got) == sorted(FIELDS), (where, type(got))
    for k in FIELDS:
        g, x = got[k], exp[k]
        assert g.dtype == x.dtype and g.shape == x.shape, (where, k, g.dtype, g.shape, x.dtype, x.shape)
        bad = np.argwhere(g != x)
        assert not len(bad), "%s: %s differs at %d of %d places, first %s: got %s expected %s" % (
            where, k, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], x[tuple(bad[0])])


def windows_move(exp, length):
    """How many executed steps leave an agent_map that differs from the block before it (a kernel that re-emits the parents' window shows none)."""
    m = exp['agent_map']
    steps = m.shape[0] - 1
    ran = np.arange(steps)[:, None] < np.asarray(length)[None, :]
    return int(((m[1:] != m[:-1]).any((2, 3)) & ran).sum())


def clipped_and_inside(exp, spec, view_size, rows_loc):
    """(windows fully inside the map, windows clipped by its edge) among the agent cells `rows_loc` [n, 2]."""
    S, V = spec.map_size, int(view_size)
    loc = np.asarray(rows_loc).reshape(-1, 2)
    inside = ((loc >= V) & (loc < S - V)).all(1)
    return int(inside.sum()), int((~inside).sum())


class OracleVecViews(TO.OracleVecTraj):
    """trajectory_oracle.OracleVecTraj whose playouts() also take observe='agent_view', view_size=: lets the adapter's, the wrappers' and the sharded
    env's forwarding of the two keywords run without a GPU.  n_items as on the device env."""

    @property
    def n_items(self):
        return len(self.spec.items_id)

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, path_keys=False, fields=None, rewards=False, masks=False, observe=None, view_size=5):
        from gym_novel_gridworlds_amd.snapshot import check_observe
        if check_observe(self, observe, view_size) != 'agent_view':
            return super().playouts(n_playouts, steps, seed, device=device, weights=weights, path_keys=path_keys, fields=fields, rewards=rewards, masks=masks,
                                    observe=observe)
        return self._playouts(n_playouts, steps, seed, weights, self._traj(path_keys, fields, rewards, masks, None,
                                                                          lambda parents, e: expect_views(self.spec, self.o.st, parents, e, view_size)))


sharded_on_oracle = functools.partial(KO.SO.T.sharded_on_oracle, OracleVecViews)
