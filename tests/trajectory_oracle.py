"""Expected trajectories from the unmodified CPU oracle.  The recorded (or given) actions of every pair are replayed once by
pairs_oracle.step_pairs (the oracle's steps on a host copy of the parents' rows), which hands back the row after every executed step;
the per-step rewards come from the same replay, the mask words from slot_observe_oracle.expect_masks on the row BEFORE each step (every action
where none would succeed), the lidar rows from slot_observe_oracle.expect_lidar on the parent and on every visited row.  Nothing here uses the
device's own step, mask or lidar code (tests/test_trajectories*.py compare the HIP path with these)."""
import functools

import numpy as np

import pairs_oracle as PA
import path_key_oracle as KO
import slot_observe_oracle as OO
from gym_novel_gridworlds_amd.state_keys import KEY_STATE

STATE_KEYS = PA.STATE_KEYS


def _stack(rows_list):
    return {k: np.stack([np.asarray(r[k]) for r in rows_list]) for k in STATE_KEYS}


def mask_words(spec, rows):
    """uint64 [n]: the valid-action word of every row of the dict `rows`, all n_actions bits where no action would succeed."""
    n = len(rows['facing'])
    m = OO.expect_masks(spec, rows, np.arange(n))
    A = m.shape[1]
    w = (m.astype(np.uint64) << np.arange(A, dtype=np.uint64)[None, :]).sum(1).astype(np.uint64)
    return np.where(w == 0, np.uint64((1 << A) - 1), w)


def observed(spec, e, lc=None, masks=True):
    """step_pairs' record (with states) as a trajectory: the record plus masks uint64 [T, count] - the word of the row BEFORE each executed step,
    unless a chooser kept its own - and obs int32 [T + 1, count, L] - the lidar rows of the parents and of every visited row - or None without a
    LidarConfig `lc`; zeros for every step a pair did not execute."""
    steps, count = e['ran'].shape
    parent_rows, states = e['parent_rows'], e['states']
    e['obs'] = None
    if masks:
        e['masks'] = np.zeros((steps, count), np.uint64)
    if lc is not None:
        first = OO.expect_lidar(spec, lc, parent_rows, np.arange(count))
        e['obs'] = np.zeros((steps + 1, count, first.shape[1]), np.int32)
        e['obs'][0] = first
    for t in range(steps):
        ran = np.nonzero(e['ran'][t])[0]
        if not ran.size:
            break
        if masks:
            before = _stack([{k: parent_rows[k][j] for k in STATE_KEYS} if t == 0 else states[(t - 1, int(j))] for j in ran])
            e['masks'][t, ran] = mask_words(spec, before)
        if lc is not None:
            after = _stack([states[(t, int(j))] for j in ran])
            e['obs'][t + 1, ran] = OO.expect_lidar(spec, lc, after, np.arange(len(ran)))
    return e


def oracle_traj(spec, rows, parents, actions, limits=None, autoreset=False, horizon=0, fields=KEY_STATE, lc=None):
    """actions int [T, count] (-1 / an id outside the list: a no-op step that counts, as in oracle_path), limits None or [count].
    -> dict(keys, reports, ends, states, events: oracle_path's five; rewards int32 [T, count]; masks uint64 [T, count]; obs int32 [T + 1, count, L]
    or None without a LidarConfig `lc`), zeros for every step a pair did not execute."""
    actions = np.asarray(actions, np.int64)
    e = observed(spec, PA.step_pairs(spec, rows, parents, actions.shape[0], actions, limits, autoreset, horizon, fields, record=True), lc)
    return {k: e[k] for k in ('keys', 'reports', 'ends', 'states', 'events', 'rewards', 'masks', 'obs')}


def widen(obs):
    """Rows of any of the three formats (an array, or the packed format's (beams, inventory) pair; numpy or torch) as one int32 array."""
    obs = OO.host(obs)
    if isinstance(obs, tuple):
        return np.concatenate([obs[0].astype(np.int32), obs[1].astype(np.int32)], -1)
    return obs.astype(np.int32)


def assert_field(got, exp, where, name):
    g = OO.host(got) if name != 'obs' else widen(got)
    if g.dtype == np.int64 and exp.dtype == np.uint64:
        g = g.view(np.uint64)
    assert g.shape == exp.shape, (where, name, g.shape, exp.shape)
    bad = np.argwhere(g != exp)
    assert not len(bad), "%s: %s differs at %d of %d places, first %s: got %s expected %s" % (
        where, name, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], exp[tuple(bad[0])])


def assert_traj(got, exp, where, fields=('rewards', 'masks', 'obs')):
    """The trajectory fields of a result equal the oracle's, bit for bit."""
    for name in fields:
        assert_field(got[name], exp[name], where, name)


class OracleVecTraj(KO.OracleVecPath):
    """path_key_oracle.OracleVecPath whose playouts() take rewards / masks / observe and whose lidar can be configured: lets the adapter's, the
    wrappers' and the sharded env's forwarding run without a GPU.  The rows come out as int32 [.., L] (the env's default lidar format)."""
    lidar, lidar_fused, lidar_packed, lidar_dtype, configured = None, False, False, np.dtype(np.int32), 0

    def lidar_configure(self, lidar_config=None, num_beams=8, fused=False, dtype=np.int32):
        from gym_novel_gridworlds_amd.lidar import LidarConfig
        self.lidar = lidar_config if lidar_config is not None else LidarConfig(self.spec, num_beams)
        self.lidar_packed = isinstance(dtype, str)
        self.lidar_dtype = np.dtype(np.uint8 if self.lidar_packed else dtype)
        self.configured += 1

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, path_keys=False, fields=None, rewards=False, masks=False, observe=None):
        from gym_novel_gridworlds_amd.snapshot import check_observe
        if not (check_observe(self, observe) or rewards or masks):
            return super().playouts(n_playouts, steps, seed, device=device, weights=weights, path_keys=path_keys, fields=fields)
        return self._playouts(n_playouts, steps, seed, weights, self._traj(path_keys, fields, rewards, masks, self.lidar if observe is not None else None))

    def _traj(self, path_keys, fields, rewards, masks, lc=None, obs_of=None):
        """The `more` of sample_oracle's _playouts for a PlayoutTraj: the fields switched on, obs_of(parents, e) in the place of the lidar rows."""
        from gym_novel_gridworlds_amd.playout import PlayoutTraj

        def more(parents, acts):
            e = oracle_traj(self.spec, self.o.st, parents, acts, None, self.o.autoreset, self.o.horizon, KEY_STATE if fields is None else fields, lc)
            return PlayoutTraj, (e['keys'] if path_keys else None, e['rewards'] if rewards else None, e['masks'] if masks else None,
                                 e['obs'] if obs_of is None else obs_of(parents, e))
        return more


sharded_on_oracle = functools.partial(KO.SO.T.sharded_on_oracle, OracleVecTraj)
