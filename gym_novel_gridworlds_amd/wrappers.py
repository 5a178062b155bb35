"""`SaveTrajectories` (gym_novel_gridworlds/wrappers.py:9-54) and `LimitActions` (:57-85) with the reference's call shape.

    env = LimitActions(env, {'Forward', 'Left', 'Right', 'Break', 'Craft_plank'})

limited id i = the i-th name of sorted(limited_actions); `action_space` shrinks to Discrete(len(limited_actions)).
On the single-env adapter it forwards like the reference wrapper (same AssertionError texts).  On a
`VecNovelGridworld` it compiles the limited table INTO the kernel's action LUT (a new batched env whose action ids are
the limited ids), so there is no per-step translation at all."""
import copy
import os
import pickle
import datetime as _datetime

import numpy as np

from . import spaces
from .novelty_wrappers import NoveltyWrapper
from .playout import forward_keywords
from .state_keys import KEY_STATE
from .vec_env import VecNovelGridworld


# What a trajectory entry holds: (key in the pickled dict, attribute of the wrapped env it is read from), in the reference's
# key order (wrappers.py:29-45); the twelfth key, "last_done", is read through the wrapper itself.
_TRAJECTORY_FIELDS = (("map_size", "map_size"), ("map", "map"), ("agent_location", "agent_location"),
                      ("agent_facing_str", "agent_facing_str"), ("block_in_front_id", "block_in_front_id"), ("items_id", "items_id"),
                      ("items_quantity", "items_quantity"), ("inventory_items_quantity", "inventory_items_quantity"),
                      ("action_str", "actions_id"), ("last_action", "last_action"))
_TRAJECTORY_FILE = "%Y-%m-%d-%H-%M-%S"                       # + "_<env_id>.bin" (wrappers.py:49)


class SaveTrajectories(NoveltyWrapper):
    """Reference wrappers.py:9-54: every step appends a snapshot of the env's public state, `save()` pickles the list to
    `<save_path>/<timestamp>_<env_id>.bin`.  Host-side bookkeeping over the single-env adapter: the snapshot's values are the
    live objects (as in the reference, entries alias `env.map` until the env rebinds it)."""

    def __init__(self, env, save_path):
        NoveltyWrapper.__init__(self, env)
        os.makedirs(save_path, exist_ok=True)
        self.save_path, self.state_trajectories = save_path, []

    def get_state(self):
        wrapped = self.env
        snapshot = {key: getattr(wrapped, attribute) for key, attribute in _TRAJECTORY_FIELDS}
        snapshot["last_done"] = self.last_done
        return snapshot

    def step(self, action_id):
        result = self.env.step(action_id)
        self.state_trajectories.append(self.get_state())
        return result

    def save(self):
        name = "%s_%s.bin" % (_datetime.datetime.now().strftime(_TRAJECTORY_FILE), self.env.env_id)
        path = os.path.join(self.save_path, name)
        with open(path, 'wb') as f:
            f.write(pickle.dumps(self.state_trajectories))
        print("Trajectories saved at: ", path)
        return path


# The two AssertionError texts of the reference's LimitActions.step (wrappers.py:76-80); the first one really reads "maxaction"
# (two string literals joined without a space).
_BAD_LIMITED_ID = "Action ID {id} is not valid, maxaction ID is {top}"
_NOT_AN_ACTION = "{name} is not a valid action for {env_id}"


class LimitActions(NoveltyWrapper):
    """Reference wrappers.py:57-85: the agent sees `len(limited_actions)` action ids, limited id i = the i-th name of
    sorted(limited_actions).  A step is two table look-ups - limited id -> name in `limited_actions_id` (the FIRST name
    holding that id, in table order: `remapaction` may install a table of its own), name -> the env's id in `actions_id`,
    read through the wrapper stack so that a remapped or extended action table below is honoured."""

    def __init__(self, env, limited_actions):
        NoveltyWrapper.__init__(self, env)
        self.limited_actions = limited_actions
        self.set_limited_actions_id(dict(zip(sorted(limited_actions), range(len(limited_actions)))))
        self.action_space = spaces.Discrete(len(limited_actions))

    def set_limited_actions_id(self, limited_actions_id):
        self.limited_actions_id = limited_actions_id

    def step(self, action_id):
        table = self.limited_actions_id
        name = next((candidate for candidate, limited in table.items() if limited == action_id), None)
        assert name is not None, _BAD_LIMITED_ID.format(id=action_id, top=len(table) - 1)
        env_actions = self.actions_id
        assert name in env_actions, _NOT_AN_ACTION.format(name=name, env_id=self.env_id)
        return self.env.step(env_actions[name])

    def action_masks(self):
        """bool [len(limited_actions)]: column i is the env's column of the action limited id i steps (the same two look-ups as step);
        a limited id step() would refuse is False."""
        return limit_mask_columns(self.env.action_masks(), self.limited_actions_id, self.actions_id, len(self.limited_actions))

    def set_agent_view(self, view_size=5, fused=True):
        """The env's set_agent_view: the AgentMap window does not depend on the action id space."""
        return self.env.set_agent_view(view_size, fused=fused)

    def agent_view(self, view_size=5, device=False, copy=False):
        """The env's agent_view, likewise passed through."""
        return self.env.agent_view(view_size, device=device, copy=copy)

    def lookahead(self, device=False, copy=False):
        """The env's lookahead table in the limited id space: column i of 'reward' / 'done' / 'result' / 'info' is the env's column of the
        action limited id i steps (the same two look-ups as step); a limited id step() would refuse is a column of zeros.  device=True:
        torch tensors on the env's device, gathered from its zero-copy views (new tensors, not views)."""
        from .vec_env import Lookahead
        n = len(self.limited_actions)
        if device:
            import torch
            t = self.env.lookahead(device=True)
            ids = limit_column_ids(self.limited_actions_id, self.actions_id, n, t['reward'].shape[-1])

            def cols(x):
                out = torch.zeros(tuple(x.shape[:-1]) + (n,), dtype=x.dtype, device=x.device)
                for i, j in enumerate(ids):
                    if j is not None:
                        out[..., i] = x[..., j]
                return out
            return Lookahead(cols(t['reward']), cols(t['done']), cols(t['result']), cols(t['info']))
        t = self.env.lookahead(copy=copy)
        cols = lambda x, dt: limit_mask_columns(x, self.limited_actions_id, self.actions_id, n, dt)   # noqa: E731
        return Lookahead(cols(t['reward'], np.int32), cols(t['done'], bool), cols(t['result'], bool), cols(t['info'], np.uint32))

    def evaluate_plans(self, plans, device=False, copy=False):
        """The env's evaluate_plans for plans written in the limited id space ([P, T] integer ids): every id goes through the same two
        look-ups as step() - as lookahead() maps columns - and an id step() would refuse raises step()'s AssertionError before anything
        runs."""
        return self.env.evaluate_plans(limit_plan_ids(plans, self.limited_actions_id, self.actions_id, len(self.limited_actions), self.env_id),
                                       device=device, copy=copy)

    def successor_keys(self, fields=KEY_STATE, device=False, reports=True):
        """The env's successor keys in the limited id space: entry i of every field is the env's entry of the action limited id i steps (the
        columns lookahead() selects); a limited id step() would refuse has key 0 and reports 0."""
        from .snapshot import SuccessorKeys
        n = len(self.limited_actions)
        t = self.env.successor_keys(fields=fields, device=device, reports=reports)
        ids = limit_column_ids(self.limited_actions_id, self.actions_id, n, t.keys.shape[-1])

        def cols(x):
            if x is None:
                return None
            if device:
                import torch
                out = torch.zeros(tuple(x.shape[:-1]) + (n,), dtype=x.dtype, device=x.device)
            else:
                out = np.zeros(x.shape[:-1] + (n,), x.dtype)
            for i, j in enumerate(ids):
                if j is not None:
                    out[..., i] = x[..., j]
            return out
        return SuccessorKeys(*[cols(x) for x in t])

    def walk_plan(self, item, steps):
        """The env's walk_plan in the limited id space: every Forward / Left / Right id of the plan as this wrapper numbers it.  ValueError if
        Forward, Left or Right is not among the limited actions.  (walk_distances() does not depend on the action id space: passed through.)"""
        ids = limit_walk_ids(self.limited_actions_id, self.actions_id)
        plan, length = self.env.walk_plan(item, steps)
        return [ids[a] for a in plan], length

    def recipe_cost(self, costs=None, scale=1):
        """The env's recipe_cost with a per-action `costs` written in the limited id space: entry i is the cost of the action limited id i steps
        (the two look-ups of step()).  An action of the env that no limited id steps costs 0 there, and so does the rule it stands for: with
        Extract_rubber outside the limited set the extraction's 50 000 drops out of the bound, with every craft and Break outside it the bound
        is 0.  That is still a lower bound - such an action cannot be taken at all - but it can collapse silently: keep the actions the recipe
        table needs in the limited set, or pass costs=None.  (Without `costs` nothing depends on the action id space: passed through.)"""
        if costs is None:
            return self.env.recipe_cost(scale=scale)
        c = np.asarray(costs)
        n = len(self.limited_actions)
        if c.dtype.kind not in 'iu' or c.shape != (n,):
            raise ValueError("costs: one integer per limited action expected, shape [%d], got dtype %s, shape %s" % (n, c.dtype, list(c.shape)))
        env_actions = self.actions_id
        full = np.zeros(self.unwrapped._backend().n_actions, np.int64)      # (the width of the batched env's action table)
        for i, j in enumerate(limit_column_ids(self.limited_actions_id, env_actions, n, len(full))):
            if j is not None:
                full[j] = c[i]
        return self.env.recipe_cost(costs=full, scale=scale)

    def _limited_env(self):
        """-> (the one-env batched env whose action table is this wrapper's list - limit_actions_vec, kept from call to call - holding a copy
        of the adapter's current state, this wrapper's id of each of its actions): what playouts() and sample_action() run on."""
        adapter = self.unwrapped
        vec = adapter._backend()
        adapter._push(vec)                                   # (attributes the caller edited since the last step go to the device first)
        env_actions = self.actions_id
        names = sorted(self.limited_actions)
        for name in names:
            assert name in env_actions, _NOT_AN_ACTION.format(name=name, env_id=self.env_id)
        kept = self.__dict__.get('_playout_env')
        if kept is None or kept[0] is not vec or kept[1] != names:
            if kept is not None:
                kept[2].close()
            kept = self.__dict__['_playout_env'] = (vec, names, limit_actions_vec(vec, names))
        limited = kept[2]
        st = vec.get_state()
        limited.set_state(0, map=st['map'], loc=st['loc'], facing=st['facing'], inv=st['inv'], selected=st['selected'], step_count=st['step_count'])
        return limited, [self.limited_actions_id[name] for name in names]

    def sample_action(self, weights, seed, t=0):
        """The env's sample_action under this wrapper's action list: weights has one entry per limited id, the action is drawn among the
        LIMITED actions that would succeed and is a limited id; bit i of the mask word is limited id i.  Runs where playouts() runs."""
        w = np.asarray(weights)
        if w.shape != (len(self.limited_actions),):
            raise ValueError("weights: one weight per limited action expected, shape [%d], got %s" % (len(self.limited_actions), list(w.shape)))
        limited, ids = self._limited_env()
        s = limited.sample_actions(w[ids][None], seed, t=t)          # (the kernel's action i is this wrapper's ids[i])
        word = sum(1 << ids[i] for i in range(len(ids)) if (int(s.mask_words[0]) >> i) & 1)
        return ids[int(s.action[0])], float(s.mass[0]), word

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, path_keys=False, fields=None, rewards=False, masks=False, observe=None,
                 view_size=5, table=None, table_weights=None, outside='default'):
        """The env's playouts under this wrapper's action list: at every step the action is drawn among the LIMITED actions that would
        succeed (every limited action where none would), and 'first_action' holds limited ids.  The draw needs the limited list as the
        kernel's own action table, so the playouts run on a one-env batched env whose table is the limited one (limit_actions_vec, kept
        from call to call) holding a copy of the current state; they equal what limit_actions_vec() of a batched env gives for that
        state.  weights: one per limited id.  path_keys / fields: as on the env - the keys do not depend on the action id space.
        rewards / masks / observe: as on the env; bit i of a mask word is limited id i, consistent with the actions reported here.  observe needs
        the lidar configured on the adapter's batched backend (the limited env takes its configuration over).  observe='agent_view' / view_size:
        the AgentMap dict, which does not depend on the action id space and needs no lidar.
        table / table_weights / outside: a guided playout.  The table is one of the LIMITED env (lim.key_table(capacity): keys do not depend on
        the action id space, tables belong to an env).  The columns of table_weights [table.buckets, n_limited] are in this wrapper's id space;
        where the kernel's order differs they are scattered to the env's columns on the device once per call - one gather over buckets * n_limited
        floats and a second tensor of that size, whatever the number of playouts - so keep the ids in sorted-name order (the default) in a loop."""
        limited, ids = self._limited_env()
        if table_weights is not None and ids != list(range(len(ids))):
            table_weights = limit_weight_columns(table_weights, ids, limited)
        if weights is not None and not hasattr(weights, 'data_ptr'):        # (a host array; numpy 2 arrays have a `device` too)
            w = np.asarray(weights)
            if w.shape != (len(ids),):
                raise ValueError("weights: one weight per limited action expected, shape [%d], got %s" % (len(ids), list(w.shape)))
            weights = w[ids]                                 # (the kernel's action i is this wrapper's ids[i])
        elif weights is not None and ids != list(range(len(ids))):
            import torch
            weights = weights[torch.tensor(ids, device=weights.device)].contiguous()
        path = forward_keywords(path_keys, fields, rewards, masks, observe, view_size, table, table_weights, outside)
        if observe is not None and not (isinstance(observe, str) and observe == 'agent_view'):   # (the views need no lidar) the rows are the backend's: its lidar as it is configured NOW, not as it was when the limited env was made
            vec = self.unwrapped._backend()
            mine, theirs = [(e.lidar, e.lidar_packed, e.lidar_dtype) for e in (limited, vec)]
            if vec.lidar is not None and mine != theirs:
                limited.lidar_configure(vec.lidar, fused=False, dtype='packed' if vec.lidar_packed else vec.lidar_dtype)
            elif vec.lidar is None:
                limited.lidar = None                         # (observe then raises what it raises on the env)
        play = limited.playouts(n_playouts, steps, seed, device=device, weights=weights, **path).row(0)
        if ids == list(range(len(ids))):
            return play
        if masks:                                            # (the kernel's bit i is this wrapper's bit ids[i])
            play = play._replace(masks=limit_mask_words(play.masks, ids))
        if device:                                           # (a table of its own, set_limited_actions_id: the kernel's id i is this wrapper's ids[i])
            import torch
            lut = torch.tensor(ids, dtype=play.first_action.dtype, device=play.first_action.device)
            return play._replace(first_action=lut[play.first_action.long()])
        return play._replace(first_action=np.asarray(ids, np.int32)[play.first_action])

    def key_table(self, capacity, values=False, **kw):
        """A key table for guided playouts() under this wrapper: VecNovelGridworld.key_table on the limited env the playouts run on.  It lives as
        long as that env does (until close(), or until the adapter's backend is rebuilt)."""
        return self._limited_env()[0].key_table(capacity, values, **kw)

    def close(self):
        kept = self.__dict__.pop('_playout_env', None)
        if kept is not None:
            kept[2].close()
        return self.env.close()

    # (state_key() is NoveltyWrapper's forward: a key describes the state, not the action ids, so it is the same on either side of this wrapper)


def limit_plan_ids(plans, limited_actions_id, actions_id, n, env_id=''):
    """Plans written in LimitActions' id space -> the env's ids: every id through the two look-ups of step() (limit_column_ids, as the
    columns of a lookahead table map).  An id step() would refuse - no name holds it, or the env does not know the name, e.g. an action
    a wrapper below removed - raises step()'s AssertionError for it."""
    plans = np.asarray(plans)
    assert plans.dtype.kind in 'iu', "plans are integer action ids"
    used = [int(i) for i in np.unique(plans)]
    ids = limit_column_ids(limited_actions_id, actions_id, max(used + [n - 1]) + 1, max(list(actions_id.values()) + [0]) + 1)
    out = np.zeros(plans.shape, np.int32)
    for i in used:
        name = next((candidate for candidate, limited in limited_actions_id.items() if limited == i), None)
        assert name is not None, _BAD_LIMITED_ID.format(id=i, top=len(limited_actions_id) - 1)
        assert ids[i] is not None, _NOT_AN_ACTION.format(name=name, env_id=env_id)
        out[plans == i] = ids[i]
    return out


def limit_walk_ids(limited_actions_id, actions_id):
    """{the env's id: LimitActions' id} of Forward, Left and Right - what a walk plan written in the env's ids is translated with.  ValueError
    where one of the three is not among the limited actions (or the env does not know it)."""
    ids = {}
    for name in ('Forward', 'Left', 'Right'):
        if name not in limited_actions_id or name not in actions_id:
            raise ValueError("walk_plan: %s is not among the limited actions %s" % (name, sorted(limited_actions_id)))
        ids[actions_id[name]] = limited_actions_id[name]
    return ids


def limit_column_ids(limited_actions_id, actions_id, n, width):
    """For each limited id i < n, the env's column it steps: the env's id (in `actions_id`) of the FIRST name that holds limited id i in
    `limited_actions_id` (table order); None where step() would refuse the id or the env has no such column (< width)."""
    ids = []
    for i in range(n):
        name = next((candidate for candidate, limited in limited_actions_id.items() if limited == i), None)
        ok = name is not None and name in actions_id and actions_id[name] < width
        ids.append(actions_id[name] if ok else None)
    return ids


def limit_mask_columns(inner, limited_actions_id, actions_id, n, dtype=bool):
    """The env's mask row(s) `inner` ([..., n_env_actions]) in LimitActions' id space: column i <- the env's column limited id i steps
    (limit_column_ids).  dtype: the columns of a lookahead table map the same way (a limited id step() would refuse is a column of
    zeros)."""
    inner = np.asarray(inner, dtype)
    out = np.zeros(inner.shape[:-1] + (n,), dtype)
    for i, j in enumerate(limit_column_ids(limited_actions_id, actions_id, n, inner.shape[-1])):
        if j is not None:
            out[..., i] = inner[..., j]
    return out


def limit_weight_columns(table_weights, ids, limited=None):
    """Weight rows [buckets, n] whose column ids[i] belongs to a wrapper's limited id ids[i] -> the rows in the kernel's order (column i <- column
    ids[i]).  A torch tensor is gathered where it lies; a host array goes to `limited`'s device first (one upload) and is gathered there - without
    `limited`, on the host."""
    if hasattr(table_weights, 'data_ptr'):
        import torch
        return table_weights[:, torch.tensor(ids, device=table_weights.device)].contiguous()
    w = np.asarray(table_weights)
    if w.ndim != 2 or w.shape[1] != len(ids):
        raise ValueError("table_weights: one column per limited action expected, shape [buckets, %d], got %s" % (len(ids), list(w.shape)))
    if limited is None or not hasattr(limited, 'device') or not hasattr(limited, '_h'):
        return np.ascontiguousarray(w[:, ids])
    import torch
    dev = torch.device('cuda:%d' % limited.device)
    return torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev)[:, torch.tensor(ids, device=dev)].contiguous()


def limit_mask_words(words, ids):
    """Mask words of an env whose action i is a wrapper's limited id ids[i] -> the words in the wrapper's id space (bit i moves to bit ids[i]).
    numpy uint64, or torch int64 over the same bits."""
    out = words * 0
    for i, j in enumerate(ids):
        out = out | (((words >> i) & 1) << j)
    return out


def limited_spec(spec, limited_actions):
    """A copy of `spec` whose action list is `limited_actions` in sorted order: limit_actions_vec's spec edit."""
    spec = copy.deepcopy(spec)
    limited = {action: i for i, action in enumerate(sorted(limited_actions))}
    for action in limited:
        assert action in spec.actions_id, action + " is not a valid action for " + spec.env_id
    spec.actions_id.clear()
    spec.actions_id.update(limited)
    spec.manipulation_actions_id = {a: i for a, i in limited.items() if not a.startswith(('Craft_', 'Select_'))}
    spec.craft_actions_id = {a: i for a, i in limited.items() if a.startswith('Craft_')}
    spec.select_actions_id = {a: i for a, i in limited.items() if a.startswith('Select_')}
    spec.action_space_n = len(limited)
    return spec


def limit_actions_vec(venv, limited_actions):
    """Batched form: a new VecNovelGridworld whose action ids ARE the limited ids (LUT edit, no translation pass)."""
    assert isinstance(venv, VecNovelGridworld)
    spec = limited_spec(venv.spec, limited_actions)
    # (the prepared-episode settings travel as the caller CHOSE them: 'auto' stays adaptive on the derived env)
    new = VecNovelGridworld(spec=spec, num_envs=venv.num_envs, device=venv.device, seed=venv.seed, autoreset=venv.autoreset,
                            horizon=venv.horizon, env_index_base=venv.env_index_base, reset_prefetch=venv._prefetch_arg,
                            reset_prefetch_depth=venv._depth_arg, terminal_capture=venv.terminal_capture)
    if venv.lidar is not None:                              # the observation setup travels with the env
        new.lidar_configure(venv.lidar, fused=venv.lidar_fused, dtype='packed' if venv.lidar_packed else venv.lidar_dtype)
    return new
