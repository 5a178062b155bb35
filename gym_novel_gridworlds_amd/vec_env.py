"""VecNovelGridworld - N concurrent environments on one MI355X behind the reference's step()/reset() contract.

Batched mirror of the reference `gym.Env` surface (gym_novel_gridworlds/envs/pogostick_v1_env.py):
`reset()` :86, `step(action_id)` :230 -> `(obs, reward, done, info)`, `get_observation()` :214 with the Dict
observation of map / agent_location / agent_facing_id / inventory_items_quantity, plus `inject_novelty`
semantics through `novelty=`.  All computation happens in the HIP kernels behind the C-ABI (`_cabi.py`)."""
import collections
import ctypes as C

import numpy as np

from . import _cabi
from .novelty import apply_novelty
from .spec import F_INVALID_ACTION, F_PLACEMENT, STEP_COSTS, EnvSpec, make_spec
from .state_keys import KEY_STATE, check_fields

_COST_F64 = np.array([float(c) for c in STEP_COSTS], np.float64)
PLACEMENT_MESSAGE = "Cannot place items, increase map size!"          # pogostick_v1_env.py:167


class _Keeper:
    """Holds the index list a queued launch may still be reading (snapshot.enqueue_ordered)."""
    _keep = None


class _DevArray:
    """Zero-copy view of a device buffer for torch.as_tensor (CUDA array interface, also honoured on ROCm)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False),
                                         'version': 2, 'strides': None}


def check_view_size(view_size):
    """The view_size of set_agent_view: an integer in 1 .. 127 (ngw_agent_view's range), as an int."""
    if isinstance(view_size, bool) or not isinstance(view_size, (int, np.integer)) or not 1 <= view_size <= 127:
        raise ValueError("view_size: an integer in 1..127 expected, got %r" % (view_size,))
    return int(view_size)


def unpack_action_masks(words, n_actions):
    """[N] packed action-mask words (bit a of word i: step(a) from env i's state would report result == True) -> bool [N, n_actions]."""
    w = np.ascontiguousarray(words, np.uint64).reshape(-1)
    bits = w.view(np.uint8).reshape(-1, 8)                  # little-endian: byte j holds actions 8j .. 8j+7
    return np.unpackbits(bits, axis=1, bitorder='little')[:, :n_actions].astype(bool)


def unpack_action_masks_device(words, n_actions):
    """unpack_action_masks with torch ops: a torch int64 tensor [N] of the same words -> a bool tensor [N, n_actions] on its device."""
    import torch
    bits = torch.arange(n_actions, device=words.device, dtype=torch.int64)
    return ((words[:, None] >> bits) & 1).bool()


def decode_info_words(words):
    """Packed info words (include/ngw.h NGW_INFO_*) of any shape -> a StepInfo that decodes 'result', 'step_cost_code', 'message_code',
    'message_arg' and 'step_cost' when they are read: what VecNovelGridworld.step_costs / .messages take.  For a lookahead table hand in
    one column (`info[:, a]`, with actions = a) or one row (`info[i]`, with actions = range(A))."""
    return StepInfo({'_words': np.asarray(words, np.uint32)})


class Lookahead(collections.namedtuple('Lookahead', 'reward done result info')):
    """What lookahead() returns: reward int32, done bool, result bool, info uint32 words, each [N, A] ([A] on the single-env adapter).
    A named tuple (it unpacks in that order) whose fields can also be read by name: t['reward']."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    def row(self, i):
        """Env i's rows (the single-env adapter's view)."""
        return Lookahead(*[x[i] for x in self])


class PlanEval(collections.namedtuple('PlanEval', 'ret length ended info')):
    """What evaluate_plans() returns: ret int32 (sum of the executed steps' rewards), length int32 (steps executed, 1 .. T), ended bool (the
    plan stopped at an episode end) and info uint32 (the packed word of the last executed step), each [N, P] ([P] on the single-env adapter).
    A named tuple (it unpacks in that order) whose fields can also be read by name: e['ret'].  numpy arrays or torch tensors."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    @property
    def goal(self):
        """The plan ended by reaching the goal (info bit 1; clear for a horizon cut)."""
        return self.ended & (((self.info >> 1) & 1) != 0)

    @property
    def died(self):
        """The plan ended in a FireWall death (message code 14)."""
        return self.ended & (((self.info >> 8) & 255) == 14)

    def row(self, i):
        """Env i's rows (the single-env adapter's view)."""
        return PlanEval(*[x[i] for x in self])


class RolloutPath(collections.namedtuple('RolloutPath', 'ret length ended info keys')):
    """What Snapshot.rollout(path_keys=True) returns: PlanEval's 'ret', 'length', 'ended' and 'info', each [count], and 'keys' [T, count]:
    entry (t, j) the key (state_keys) of the state pair j is in after it has executed step t, 0 for a step it did not execute - numpy
    uint64, or a torch int64 tensor over the same bits.  A named tuple whose fields can also be read by name: r['keys']."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    goal = PlanEval.goal
    died = PlanEval.died


class RolloutTraj(collections.namedtuple('RolloutTraj', 'ret length ended info keys rewards obs')):
    """What Snapshot.rollout(rewards=True / observe='lidar') returns: RolloutPath's fields ('keys' None without path_keys) and, each None where
    it was not asked for, 'rewards' int32 [T, count] (the reward of step t of pair j, 0 for a step it did not execute: rewards.sum(0) == ret) and
    'obs' [T + 1, count, row] in the env's lidar format (obs[0] the parents, obs[t + 1] the state step t leaves, zero rows for steps not executed;
    the packed format: the pair (beams, inventory)) - see playout.PlayoutTraj."""
    __slots__ = ()

    def __getitem__(self, key):
        return getattr(self, key) if isinstance(key, str) else tuple.__getitem__(self, key)

    goal = PlanEval.goal
    died = PlanEval.died


class StepInfo(dict):
    """info of a batched step: 'result' bool[N], 'step_cost_code', 'message_code', 'message_arg' - and 'step_cost' f64[N].  Fields
    that are not there yet are made when they are first asked for: 'step_cost' is looked up from the codes (a 65 536-element
    gather per step costs more than the step kernel; few callers read it), and on big batches all four code arrays are
    decoded from the packed info words ('_words', include/ngw.h NGW_INFO_*) only then - the C-side decode of 65 536 words
    costs 40 us per step, and a rollout loop reads reward and done.  Behaves as a dict that has the keys."""
    __slots__ = ()
    LAZY = ('result', 'step_cost_code', 'message_code', 'message_arg', 'step_cost')

    def __missing__(self, key):
        if key == 'final_observation' and dict.__contains__(self, '_final_fn'):      # terminal observations (set_terminal_capture): fetched when asked for
            v = dict.__getitem__(self, '_final_fn')()
            dict.__setitem__(self, key, v)
            return v
        if key in StepInfo.LAZY:
            if key == 'step_cost':
                v = _COST_F64[self['step_cost_code']]
            else:
                w = dict.__getitem__(self, '_words')
                v = {'result': lambda: (w & 1).astype(np.bool_), 'step_cost_code': lambda: ((w >> 2) & 63).astype(np.uint8),
                     'message_code': lambda: ((w >> 8) & 255).astype(np.uint16), 'message_arg': lambda: (w >> 16).astype(np.uint16)}[key]()
            dict.__setitem__(self, key, v)
            return v
        raise KeyError(key)

    def __contains__(self, key):
        return key in StepInfo.LAZY or dict.__contains__(self, key) or (key == 'final_observation' and dict.__contains__(self, '_final_fn'))

    def get(self, key, default=None):
        return self[key] if key in self else default

    def _all(self):
        for k in StepInfo.LAZY:
            self[k]
        return self

    def keys(self):
        return [k for k in dict.keys(self._all()) if k not in ('_words', '_final_fn')]

    def items(self):
        return [(k, v) for k, v in dict.items(self._all()) if k not in ('_words', '_final_fn')]

    def values(self):
        return [v for k, v in dict.items(self._all()) if k not in ('_words', '_final_fn')]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def copy(self):
        return StepInfo(dict(self.items()))


class LazyObs(dict):
    """The Dict observation of a big batch's step(): 'map' and 'inventory_items_quantity' are sections of the page-locked block the
    step refreshes; the agent's pose crosses PCIe as four bytes per env (ngw_step_host_packed) and 'agent_location' [N, 2] int32 /
    'agent_facing_id' [N] int32 are widened from those bytes into the same two arrays when somebody reads them (a 65 536-env widening
    costs more than the step kernel; a loop that feeds a policy from the map or the lidar rows never asks).  A dict in every other way."""
    __slots__ = ('_pose', '_dirty')

    def _sync(self):
        if self._dirty:
            self._dirty = False
            pose = self._pose
            loc = dict.__getitem__(self, 'agent_location')
            loc[:, 0] = pose[:, 0]
            loc[:, 1] = pose[:, 1]
            dict.__getitem__(self, 'agent_facing_id')[:] = pose[:, 2]

    def __getitem__(self, key):
        if key != 'map' and key != 'inventory_items_quantity':
            self._sync()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        self._sync()
        return dict.items(self)

    def values(self):
        self._sync()
        return dict.values(self)

    def copy(self):
        self._sync()
        return dict(dict.items(self))

    # dict(obs), {**obs}, other.update(obs), np.savez(**obs): CPython merges a dict SUBCLASS through the fast path that bypasses
    # __getitem__ unless the subclass overrides __iter__ - with these two the merge walks keys() + __getitem__, which sync
    def __iter__(self):
        self._sync()
        return dict.__iter__(self)

    def keys(self):
        self._sync()
        return dict.keys(self)


class VecNovelGridworld:
    def __init__(self, env_id='NovelGridworld-Pogostick-v1', num_envs=1, map_size=None, novelty=None, device=0,
                 seed=0, autoreset=False, horizon=0, env_index_base=0, spec=None, reset_prefetch='auto', reset_prefetch_depth=0,
                 terminal_capture=False):
        if spec is None:
            spec = make_spec(env_id, map_size)
            if novelty:
                novs = [novelty] if isinstance(novelty[0], str) else list(novelty)
                for nv in novs:
                    apply_novelty(spec, *nv)
        assert isinstance(spec, EnvSpec)
        self.num_envs = int(num_envs)
        self.device = int(device)
        self.seed = int(seed)
        self.env_index_base = int(env_index_base)
        self.autoreset, self.horizon = bool(autoreset), int(horizon)
        # what the caller chose for the prepared next episodes ('auto' / 0 = the library's own defaults); rebuild() re-applies it
        self._prefetch_arg, self._depth_arg = reset_prefetch, int(reset_prefetch_depth)
        self.terminal_capture = bool(terminal_capture)         # keep the observation an episode ENDED in (set_terminal_capture)
        self.lidar, self.lidar_fused, self.lidar_len, self.lidar_dtype, self.lidar_packed = None, False, 0, np.dtype(np.int16), False   # set by lidar_configure()
        self._h = C.c_void_p()
        self._open(spec)

    def _open(self, spec):
        """Create the device handle for `spec` and apply this env's settings to it."""
        self.spec = spec
        self.cspec = spec.compile()
        self.map_size = spec.map_size
        self.n_items = len(spec.items_id)
        self.items_id = dict(spec.items_id)
        self.actions_id = dict(spec.actions_id)
        self.single_action_space_n = spec.action_space_n
        from . import spaces
        self.action_space = spaces.Discrete(spec.action_space_n)           # per env; NOT grown by axe/additem
        self.observation_space = spaces.Dict({'map': spaces.Box(low=0, high=spec.max_items, shape=(spec.map_size, spec.map_size, 1))})
        import os
        self._zc_bytes = int(os.environ.get('NGW_ZC_BYTES', 256 << 10)) or 1     # (read where ngw_create reads it)
        L = _cabi.lib()
        _cabi.check(L.ngw_create(C.byref(self.cspec), self.num_envs, self.device, self.seed, self.env_index_base,
                                 C.byref(self._h)))
        _cabi.check(L.ngw_set_autoreset(self._h, int(self.autoreset), self.horizon))
        # 'auto' = the library's own default: ngw_set_autoreset switched prepared next episodes on (a refill every 3/4 horizon)
        # unless the episodes are too short for that cadence to keep up (rows would go stale and resets simply run inline)
        self.reset_prefetch = self._default_prefetch()
        self._prefetch_user = False
        if self._depth_arg:
            self.set_reset_prefetch_depth(self._depth_arg)
        if self._prefetch_arg != 'auto':
            self.set_reset_prefetch(self._prefetch_arg)
        self._flags_word = C.c_uint32(0)
        self._host = None                                     # host mirrors of the host API: allocated on first use
        if self.__dict__.get('_stream_arg'):                  # the caller's stream and output bindings travel with the env (rebuild)
            self.set_stream(self._stream_arg)
        if self.__dict__.get('_rollout_out_args'):
            self.rollout_outputs(*self._rollout_out_args)
        if self.terminal_capture:
            self.set_terminal_capture(True)
        if self.lidar is not None:                            # the observation setup travels with the env (rebuild)
            self.lidar_configure(self.lidar, fused=self.lidar_fused, dtype='packed' if self.lidar_packed else self.lidar_dtype)
        if self.__dict__.get('_act_masks_on'):
            self.set_action_masks(True)
        if self.__dict__.get('_agent_view_cfg'):
            self.set_agent_view(*self._agent_view_cfg)

    def rebuild(self, spec):
        """The same batched env - same object, same shard of the global env index space (`env_index_base`), same autoreset /
        horizon / prepared-episode / lidar / terminal-capture settings, same stream and rollout-output bindings - on an edited spec.
        In place: the reference's novelty wrappers mutate the env they wrap and keep its identity (novelty_wrappers.py:1586-1674), so a
        rank-local shard stays that shard.  The NEW handle is created first: a spec the library refuses (ngw_create's checks) raises
        and leaves the env as it was - the reference, too, asserts before it changes anything.  The state is undefined until the
        next reset(), as after construction."""
        old_h, old_attrs = self._h, dict(self.__dict__)
        for name in VecNovelGridworld._HOST_ATTRS + ('_host', '_step_args', '_step1_args', '_step1_fn', '_step1_mv', '_state1_mv', '_reset1_args', '_last_state_views', '_lidar_host', '_view_host', '_plan_stage', '_plan_host', '_last_actions', '_packed_block', '_packed_call', '_steps_stale'):
            self.__dict__.pop(name, None)
        self._h = C.c_void_p()
        try:
            self._open(spec)
        except Exception:
            if self._h:
                _cabi.lib().ngw_destroy(self._h)
            self.__dict__.clear()
            self.__dict__.update(old_attrs)                   # the old handle, spec and host mirrors: nothing happened
            raise
        if old_h:
            _cabi.lib().ngw_destroy(old_h)                    # (waits for the old handle's stream)
        self._drop_snapshots(sync=False)                      # they held states in the old handle's map size and item count, and went with it
        return self

    _HOST_ATTRS = ('_obs', '_reward', '_done', '_act_pinned', '_sel_host', '_steps_host', '_result', '_cost', '_msg', '_arg', '_flags_np', '_info_words')

    def __getattr__(self, name):
        # The host mirrors (10 MB page-locked at 65 536 envs, 157 B per env) exist only for the host API; a handle that is
        # only ever driven through device pointers (step_device / rollout / device_observation) never pays for them.
        if name in VecNovelGridworld._HOST_ATTRS:
            if self.__dict__.get('_host') is None:
                N, S, K = self.num_envs, self.map_size, self.n_items
                if self._one_block_path():
                    self._make_packed_host()
                    return self.__dict__[name]
                # ONE page-locked block laid out as ngw_host_step_layout says: a big batch's step() then comes back with a single
                # copy across PCIe (one pack launch on the device) instead of nine
                offs = (C.c_uint64 * 11)()
                _cabi.check(_cabi.lib().ngw_host_step_layout(self._h, offs))
                block = _cabi.pinned_array((int(offs[10]),), np.uint8)

                def sec(i, shape, dt):
                    nb = int(np.prod(shape)) * np.dtype(dt).itemsize
                    return block[int(offs[i]):int(offs[i]) + nb].view(dt).reshape(shape)
                self.__dict__['_host'] = dict(
                    _obs={'map': sec(0, (N, S, S), np.int8), 'agent_location': sec(1, (N, 2), np.int32),
                          'agent_facing_id': sec(2, (N,), np.int32), 'inventory_items_quantity': sec(3, (N, K), np.int32)},
                    _reward=sec(4, (N,), np.int32), _done=sec(5, (N,), np.uint8), _flags_np=sec(7, (1,), np.uint32),
                    # the packed info words of the last step(): big batches (the one-block path of ngw_step_host) decode them lazily
                    _info_words=sec(6, (N,), np.uint32) if self._one_block_path() else None,
                    _sel_host=sec(8, (N,), np.uint8), _steps_host=sec(9, (N,), np.int32),     # selected item / step_count after the last step()
                    _act_pinned=_cabi.pinned_array((N,), np.int32),
                    _result=np.zeros(N, np.uint8), _cost=np.zeros(N, np.uint8), _msg=np.zeros(N, np.uint16), _arg=np.zeros(N, np.uint16))
                self.__dict__.update(self.__dict__['_host'])   # plain attributes from now on (no __getattr__ detour per access)
            return self.__dict__[name]
        raise AttributeError(name)

    def _make_packed_host(self):
        """Host mirrors of a big batch: ONE page-locked block in the narrow wire format (include/ngw.h ngw_host_step_layout_packed) -
        map and inventory refreshed by deltas, pose as four bytes per env, reward int32, done uint8, packed info words."""
        N, S, K = self.num_envs, self.map_size, self.n_items
        offs = (C.c_uint64 * 8)()
        _cabi.check(_cabi.lib().ngw_host_step_layout_packed(self._h, offs))
        block = _cabi.pinned_array((int(offs[7]),), np.uint8)

        def sec(i, shape, dt):
            nb = int(np.prod(shape)) * np.dtype(dt).itemsize
            return block[int(offs[i]):int(offs[i]) + nb].view(dt).reshape(shape)
        pose = sec(2, (N, 4), np.uint8)
        obs = LazyObs({'map': sec(0, (N, S, S), np.int8), 'agent_location': np.zeros((N, 2), np.int32),
                       'agent_facing_id': np.zeros(N, np.int32), 'inventory_items_quantity': sec(1, (N, K), np.int32)})
        obs._pose, obs._dirty = pose, False
        self.__dict__['_host'] = dict(
            _obs=obs, _reward=sec(3, (N,), np.int32), _done=sec(4, (N,), np.uint8), _info_words=sec(5, (N,), np.uint32), _flags_np=sec(6, (1,), np.uint32),
            _sel_host=pose[:, 3], _steps_host=np.zeros(N, np.int32), _act_pinned=np.zeros(N, np.int32),
            _result=np.zeros(N, np.uint8), _cost=np.zeros(N, np.uint8), _msg=np.zeros(N, np.uint16), _arg=np.zeros(N, np.uint16))
        self.__dict__.update(self.__dict__['_host'])
        self.__dict__['_packed_block'] = block
        self.__dict__['_steps_stale'] = False

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._drop_snapshots()                            # (ngw_destroy frees their buffers)
            _cabi.lib().ngw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass

    def set_autoreset(self, autoreset, horizon=0):
        self.autoreset, self.horizon = bool(autoreset), int(horizon)
        _cabi.check(_cabi.lib().ngw_set_autoreset(self._h, int(self.autoreset), self.horizon))
        if not self.__dict__.get('_prefetch_user'):
            self.reset_prefetch = self._default_prefetch()

    def set_stream(self, hip_stream_ptr):
        _cabi.check(_cabi.lib().ngw_set_stream(self._h, C.c_void_p(hip_stream_ptr)))
        self._stream_arg = hip_stream_ptr                     # (rebuild() puts the new handle on the same stream)

    def stream_order(self, other_stream_ptr, handle_waits):
        """Order this env's stream and another HIP stream behind each other without a host wait (include/ngw.h ngw_stream_order)."""
        _cabi.check(_cabi.lib().ngw_stream_order(self._h, C.c_void_p(int(other_stream_ptr)) if other_stream_ptr else None, int(bool(handle_waits))))

    # ------------------------------------------------------------------ reference surface, batched
    def reset(self, mask=None, copy=False):
        """reset() for all envs (or mask != 0).  Returns the Dict observation (host arrays)."""
        self._lidar_rows_fresh = False
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            assert m.shape == (self.num_envs,)
        _cabi.check(_cabi.lib().ngw_reset(self._h, _cabi._ptr(m, np.uint8)))
        self._raise_flags()
        return self.get_observation(copy)

    def reset1(self):
        """reset() of a one-env handle for the gym.Env adapter: one C-ABI call (ngw_reset_host) that fills the host mirrors
        last_state() shows; a placement that cannot succeed raises like reset()."""
        self._lidar_rows_fresh = False
        args = self.__dict__.get('_reset1_args')
        if args is None:
            assert self.num_envs == 1
            o, p = self._obs, _cabi._ptr
            args = self._reset1_args = (self._h, None, p(o['map'], np.int8), p(o['agent_location'], np.int32), p(o['agent_facing_id'], np.int32),
                                        p(o['inventory_items_quantity'], np.int32), p(self._sel_host, np.uint8), p(self._steps_host, np.int32),
                                        p(self._flags_np, np.uint32))
        rc = _cabi.lib().ngw_reset_host(*args)
        if rc:
            _cabi.check(rc)
        if self._flags_np[0]:
            self._raise_flags()

    def step(self, actions, copy=False, with_obs=True):
        """step(action_id) for every env: (obs, reward[N] i32, done[N] bool, info) with host arrays.
        `with_obs=False` leaves the Dict observation on the device (obs is None): observation wrappers that return their
        own observation (LidarInFront, AgentMap) use it to skip the largest copy of the call.

        info = {'result' bool[N], 'step_cost' f64[N], 'step_cost_code', 'message_code', 'message_arg'};
        `messages(info, actions)` formats the reference's strings lazily."""
        a = np.ascontiguousarray(actions, np.int32)
        assert a.shape == (self.num_envs,)
        o = self._obs
        block = self.__dict__.get('_packed_block')
        if block is not None:
            # big batch, narrow wire format (ngw_step_host_packed): the actions are narrowed to bytes on their way into a buffer the step
            # kernel reads in place, map / inventory come back as deltas, pose + reward + done + info as 11 B per env in one copy
            fn = self.__dict__.get('_packed_call')
            if fn is None:                                            # (the library entry and the block's pointer: looked up / built once)
                fn = self.__dict__['_packed_call'] = (_cabi.lib().ngw_step_host_packed, _cabi._ptr(block, np.uint8))
            rc = fn[0](self._h, a.ctypes.data, fn[1], 1 if with_obs else 0)
            if rc:
                _cabi.check(rc)
            self._last_actions = a
            o._dirty = True
            self._steps_stale = True
            self._lidar_rows_fresh = self.lidar_fused                  # (ngw_lidar_host_rows: the rows of this state are in the host buffer)
            obs = None if not with_obs else ({k: v.copy() for k, v in o.items()} if copy else o)
            reward, done = (self._reward.copy(), self._done.view(np.bool_).copy()) if copy else (self._reward, self._done.view(np.bool_))
            info = StepInfo({'_words': self._info_words.copy() if copy else self._info_words})
            if self._flags_np[0]:
                self._raise_flags()
            if self.terminal_capture:
                dict.__setitem__(info, '_final_fn', self.terminal_observation)
                info['_final_observation'] = done
            return obs, reward, done, info
        self._lidar_rows_fresh = False
        self._act_pinned[...] = a
        cache = self.__dict__.setdefault('_step_args', {})
        args = cache.get(bool(with_obs))
        if args is None:                                             # the host arrays never move: the argument list is built once
            p = _cabi._ptr
            lazy = with_obs and self._info_words is not None         # big batch, one-block path: info decoded on demand from the words
            args = cache[bool(with_obs)] = (
                self._h, p(self._act_pinned, np.int32), p(o['map'], np.int8) if with_obs else None, p(o['agent_location'], np.int32),
                p(o['agent_facing_id'], np.int32), p(o['inventory_items_quantity'], np.int32), p(self._reward, np.int32),
                p(self._done, np.uint8), None if lazy else p(self._result, np.uint8), None if lazy else p(self._cost, np.uint8),
                None if lazy else p(self._msg, np.uint16), None if lazy else p(self._arg, np.uint16),
                p(self._flags_np, np.uint32), p(self._sel_host, np.uint8), p(self._steps_host, np.int32))
        rc = _cabi.lib().ngw_step_host(*args)                        # actions in, launch, observation + outputs out: one sync
        if rc:
            _cabi.check(rc)
        self._last_actions = a
        obs = None if not with_obs else ({k: v.copy() for k, v in o.items()} if copy else o)
        if with_obs and self._info_words is not None:
            reward, done = (self._reward.copy(), self._done.view(np.bool_).copy()) if copy else (self._reward, self._done.view(np.bool_))
            info = StepInfo({'_words': self._info_words.copy() if copy else self._info_words})
        else:
            reward, done, info = self._step_out_views(copy)
        if self._flags_np[0]:
            self._raise_flags()
        if self.terminal_capture:                             # gym.vector convention: info['final_observation'] (rows valid where the mask is set)
            dict.__setitem__(info, '_final_fn', self.terminal_observation)
            info['_final_observation'] = done
        return obs, reward, done, info

    def set_terminal_capture(self, on=True):
        """Keep, for every env that ends an episode in a step() under autoreset, the observation that episode ENDED in (the step
        itself returns the next episode's first observation): include/ngw.h ngw_set_terminal_capture.  step() then puts
        info['_final_observation'] (= done) and a lazily fetched info['final_observation'] into its info; terminal_observation() reads
        the side set directly.  Off by default.  Fused rollouts capture too: afterwards row e is the state env e's last finished episode ended in."""
        _cabi.check(_cabi.lib().ngw_set_terminal_capture(self._h, int(bool(on))))
        self.terminal_capture = bool(on)

    def terminal_observation(self, device=False):
        """Dict observation rows of the states episodes ended in ([N, ...] arrays like get_observation(); row e is meaningful for
        the envs whose `done` the last step() set, and keeps its value until env e ends an episode again).  device=True: zero-copy
        torch views of the side set."""
        N, S, K = self.num_envs, self.map_size, self.n_items
        if device:
            import torch
            p = [C.c_void_p() for _ in range(4)]
            _cabi.check(_cabi.lib().ngw_terminal_device_ptrs(self._h, *[C.byref(x) for x in p]))
            dev = 'cuda:%d' % self.device
            return {'map': torch.as_tensor(_DevArray(p[0].value, (N, S, S), '|i1'), device=dev),
                    'agent_location': torch.as_tensor(_DevArray(p[1].value, (N, 2), '<i4'), device=dev),
                    'agent_facing_id': torch.as_tensor(_DevArray(p[2].value, (N,), '<i4'), device=dev),
                    'inventory_items_quantity': torch.as_tensor(_DevArray(p[3].value, (N, K), '<i4'), device=dev)}
        out = {'map': np.zeros((N, S, S), np.int8), 'agent_location': np.zeros((N, 2), np.int32), 'agent_facing_id': np.zeros(N, np.int32),
               'inventory_items_quantity': np.zeros((N, K), np.int32)}
        _cabi.check(_cabi.lib().ngw_get_terminal_obs(self._h, _cabi._ptr(out['map'], np.int8), _cabi._ptr(out['agent_location'], np.int32),
                                                     _cabi._ptr(out['agent_facing_id'], np.int32), _cabi._ptr(out['inventory_items_quantity'], np.int32)))
        return out

    def _one_block_path(self):
        """Does ngw_step_host take its one-block path (pack + one copy, delta refresh) for this env's full step()?  The rule of
        ngw_abi.cpp: more than one wavefront of envs and more output bytes than the zero-copy limit (NGW_ZC_BYTES, 256 KiB)."""
        n, S2, K = self.num_envs, self.map_size ** 2, self.n_items
        total = sum((b + 255) & ~255 for b in (n * S2, n * 8, n * 4, n * K * 4, n * 4, n, 4, n, n * 4))
        return n > 64 and total > self._zc_bytes

    def refresh_host(self):
        """The next step() copies the whole observation to the host again instead of only what changed since the last step()
        (include/ngw.h ngw_host_step_layout) - call it after writing into the host arrays step() returned."""
        _cabi.check(_cabi.lib().ngw_host_mirror_invalidate(self._h))

    def step1(self, action):
        """step() of a one-env handle for the gym.Env adapter: same C-ABI call, but the argument list is built once and the
        outputs come back as Python scalars: (reward, done, result, cost code, message code, message arg)."""
        self._lidar_rows_fresh = False
        args = self.__dict__.get('_step1_args')
        if args is None:
            assert self.num_envs == 1
            o, p = self._obs, _cabi._ptr
            args = self._step1_args = (
                self._h, p(self._act_pinned, np.int32), p(o['map'], np.int8), p(o['agent_location'], np.int32),
                p(o['agent_facing_id'], np.int32), p(o['inventory_items_quantity'], np.int32), p(self._reward, np.int32),
                p(self._done, np.uint8), p(self._result, np.uint8), p(self._cost, np.uint8), p(self._msg, np.uint16), p(self._arg, np.uint16),
                p(self._flags_np, np.uint32), p(self._sel_host, np.uint8), p(self._steps_host, np.int32))
            self._step1_fn = _cabi.lib().ngw_step_host
            # memoryviews of the one-element host buffers: indexing them yields Python ints without a numpy scalar in between
            self._step1_mv = tuple(memoryview(x) for x in (self._act_pinned, self._reward, self._done, self._result, self._cost, self._msg,
                                                             self._arg, self._flags_np))
        act, reward, done, result, cost, msg, arg, flags = self._step1_mv
        act[0] = action
        rc = self._step1_fn(*args)
        if rc:
            _cabi.check(rc)
        if flags[0]:
            self._raise_flags()
        return (reward[0], done[0] != 0, result[0] != 0, cost[0], msg[0], arg[0])

    def last_state1(self):
        """The one env's state after the last step1() / reset1() as plain Python values - (map row bytes, r, c, facing,
        inventory row bytes, selected item id, step_count) - read from the host buffers that call filled."""
        mv = self.__dict__.get('_state1_mv')
        if mv is None:
            assert self.num_envs == 1
            o = self._obs
            mv = self._state1_mv = (memoryview(o['map']).cast('B'), memoryview(o['agent_location']).cast('B').cast('i'),
                                    memoryview(o['agent_facing_id']), memoryview(o['inventory_items_quantity']).cast('B'),
                                    memoryview(self._sel_host), memoryview(self._steps_host))
        m, loc, fac, inv, sel, steps = mv
        return m.tobytes(), loc[0], loc[1], fac[0], inv.tobytes(), sel[0], steps[0]

    def last_state(self):
        """State after the last step() as get_state() would return it, from the host buffers that call filled (no device
        traffic; `episode` is not part of it)."""
        if self.__dict__.get('_packed_block') is not None:
            self._obs._sync()
            if self._steps_stale:                             # (step_count does not travel in the narrow wire format: fetched when asked for)
                _cabi.check(_cabi.lib().ngw_get_state(self._h, 0, self.num_envs, None, None, None, None, None, _cabi._ptr(self._steps_host, np.int32), None))
                self._steps_stale = False
        st = self.__dict__.get('_last_state_views')
        if st is None:                                        # views of the host buffers every step fills: built once
            o = self._obs
            st = self._last_state_views = dict(map=o['map'].reshape(self.num_envs, -1), loc=o['agent_location'], facing=o['agent_facing_id'],
                                               inv=o['inventory_items_quantity'], selected=self._sel_host, step_count=self._steps_host)
        return st

    def get_observation(self, copy=False):
        o = self._obs
        if isinstance(o, LazyObs):
            o._dirty = False                                  # (the pose arrays are filled from the device below)
        _cabi.check(_cabi.lib().ngw_get_obs(self._h, _cabi._ptr(o['map'], np.int8), _cabi._ptr(o['agent_location'], np.int32),
                                            _cabi._ptr(o['agent_facing_id'], np.int32),
                                            _cabi._ptr(o['inventory_items_quantity'], np.int32)))
        return {k: v.copy() for k, v in o.items()} if copy else o

    def get_step_out(self, copy=False):
        _cabi.check(_cabi.lib().ngw_get_step_out(self._h, _cabi._ptr(self._reward, np.int32), _cabi._ptr(self._done, np.uint8),
                                                 _cabi._ptr(self._result, np.uint8), _cabi._ptr(self._cost, np.uint8),
                                                 _cabi._ptr(self._msg, np.uint16), _cabi._ptr(self._arg, np.uint16)))
        return self._step_out_views(copy)

    def _step_out_views(self, copy=False):
        info = StepInfo({'result': self._result.view(np.bool_), 'step_cost_code': self._cost, 'message_code': self._msg, 'message_arg': self._arg})
        reward, done = self._reward, self._done.view(np.bool_)      # (the kernels store 0 / 1)
        if copy:
            reward, done = reward.copy(), done.copy()
            info = StepInfo({k: v.copy() for k, v in dict.items(info)})
        return reward, done, info

    def messages(self, info, actions):
        return [self.spec.format_message(int(a), int(c), int(g))
                for a, c, g in zip(actions, info['message_code'], info['message_arg'])]

    def step_costs(self, info):
        """step_cost as the reference's Python objects (float or int)."""
        return [STEP_COSTS[int(c)] for c in info['step_cost_code']]

    # ------------------------------------------------------------------ device-resident path
    def step_device(self, actions_ptr):
        """One batched step with int32 actions already in HBM (`actions_ptr` = device address, e.g. tensor.data_ptr())."""
        self._lidar_rows_fresh = False
        _cabi.check(_cabi.lib().ngw_step_device(self._h, C.c_void_p(int(actions_ptr))))

    def step_device_many(self, actions_ptr, step_stride, n_steps):
        """n_steps batched steps from one call: step i reads int32 actions at device address actions_ptr + 4 * i * step_stride."""
        self._lidar_rows_fresh = False
        _cabi.check(_cabi.lib().ngw_step_device_many(self._h, C.c_void_p(int(actions_ptr)), int(step_stride), int(n_steps)))

    def _default_prefetch(self):
        """The refill cadence the library chose for this autoreset / horizon setting (include/ngw.h ngw_set_autoreset)."""
        v = C.c_int32()
        _cabi.check(_cabi.lib().ngw_get_reset_prefetch(self._h, C.byref(v)))
        return int(v.value)

    def set_reset_prefetch(self, every_n_steps):
        """Keep every env's NEXT episode prepared in shadow buffers and re-prepare consumed ones every `every_n_steps`
        batched steps (include/ngw.h ngw_set_reset_prefetch): resets become a row copy, which matters when episode ends
        are spread over the batch (a few envs per step).  Bit-identical results; 0 switches it off."""
        _cabi.check(_cabi.lib().ngw_set_reset_prefetch(self._h, int(every_n_steps)))
        self.reset_prefetch = int(every_n_steps)
        self._prefetch_user = True
        self._prefetch_arg = int(every_n_steps)

    def set_reset_prefetch_depth(self, depth):
        """How many episodes ahead are kept prepared per env: 1, 2, 4 or 8; 0 = automatic (the default: 1, growing by itself when
        envs end episodes faster than a refill comes round).  include/ngw.h ngw_set_reset_prefetch_depth; results do not depend on it."""
        _cabi.check(_cabi.lib().ngw_set_reset_prefetch_depth(self._h, int(depth)))
        self._depth_arg = int(depth)

    @property
    def refill_cadence(self):
        """Batched steps between two refills right now (0 = prepared episodes off): under the default setting the library adapts it
        to how fast episodes end (diagnostic entry point ngw_debug_refill_cadence)."""
        f = _cabi.lib().ngw_debug_refill_cadence
        f.argtypes, f.restype = [C.c_void_p], C.c_int
        return int(f(self._h))

    @property
    def step_reads_map_in_place(self):
        """True if step launches run the kernel that reads the few map cells a step needs straight from HBM, False if they stage the
        wave's maps through LDS (include/ngw.h ngw_step_kernel_info)."""
        v = C.c_int32()
        _cabi.check(_cabi.lib().ngw_step_kernel_info(self._h, C.byref(v)))
        return bool(v.value & 1)                                     # (the word's other flags: step_kernel_plain)

    @property
    def step_kernel_plain(self):
        """(handle, last): `handle` - batched steps that bring an int32 action row run the in-place kernel's instantiation for the plain
        spec class (at most 12 items, no Jump action, no entities, one "near" item, nothing fused; NGW_STEP_PLAIN=0 switches it off);
        `last` - the last per-launch step (or the launches a graph captured) ran it.  Flags 2 and 4 of ngw_step_kernel_info's word."""
        v = C.c_int32()
        _cabi.check(_cabi.lib().ngw_step_kernel_info(self._h, C.byref(v)))
        return bool(v.value & 2), bool(v.value & 4)

    @property
    def reset_prefetch_depth(self):
        v = C.c_int32()
        _cabi.check(_cabi.lib().ngw_get_reset_prefetch_depth(self._h, C.byref(v)))
        return int(v.value)

    def rollout(self, n_steps, action_seed=1234, t0=0):
        """Fused mode: n_steps steps in one launch with on-device uniform actions."""
        self._lidar_rows_fresh = False
        _cabi.check(_cabi.lib().ngw_rollout(self._h, int(n_steps), int(action_seed), int(t0)))

    def rollout_actions(self, actions_ptr, step_stride, n_steps):
        """Fused mode with the caller's actions: n_steps steps in one launch, step t reads int32 actions at device address
        actions_ptr + 4 * t * step_stride (e.g. a [T, N] int32 tensor: data_ptr(), N, T)."""
        self._lidar_rows_fresh = False
        _cabi.check(_cabi.lib().ngw_rollout_actions(self._h, C.c_void_p(int(actions_ptr)), int(step_stride), int(n_steps)))

    def rollout_outputs(self, reward_rows_ptr=0, done_rows_ptr=0, row_stride=0, accumulate=False):
        """Per-step outputs of the fused rollouts (include/ngw.h ngw_rollout_outputs): int32 reward rows and uint8 done rows
        [T, row_stride] in device memory (0 = off), and per-env episode accumulators kept across rollout calls."""
        _cabi.check(_cabi.lib().ngw_rollout_outputs(self._h, C.c_void_p(int(reward_rows_ptr)) if reward_rows_ptr else None,
                                                    C.c_void_p(int(done_rows_ptr)) if done_rows_ptr else None, int(row_stride), int(bool(accumulate))))
        self._rollout_out_args = (reward_rows_ptr, done_rows_ptr, row_stride, accumulate)   # (rebuild() re-binds them)

    def episode_stats(self, clear=False):
        """dict of int32 [N] host arrays: return / length of the running episodes, sum of returns / count of the finished ones."""
        out = {k: np.zeros(self.num_envs, np.int32) for k in ('run_return', 'run_length', 'sum_return', 'n_episodes')}
        _cabi.check(_cabi.lib().ngw_episode_stats(self._h, *[_cabi._ptr(out[k], np.int32) for k in ('run_return', 'run_length', 'sum_return', 'n_episodes')],
                                                  int(bool(clear))))
        return out

    def sync(self):
        _cabi.check(_cabi.lib().ngw_sync(self._h))

    def error_flags(self):
        f = C.c_uint32(0)
        _cabi.check(_cabi.lib().ngw_error_flags(self._h, C.byref(f)))
        return f.value

    def _raise_flags(self):
        f = self.error_flags()
        if f & F_PLACEMENT:
            raise AssertionError(PLACEMENT_MESSAGE)
        if f & F_INVALID_ACTION:
            raise ValueError("action id outside [0, %d) is not in list" % len(self.actions_id))

    def device_observation(self):
        """Current observation buffers as torch tensors (zero copy; valid until the next step/reset)."""
        import torch
        p = [C.c_void_p() for _ in range(4)]
        _cabi.check(_cabi.lib().ngw_obs_device_ptrs(self._h, *[C.byref(x) for x in p]))
        N, S, K = self.num_envs, self.map_size, self.n_items
        dev = 'cuda:%d' % self.device
        return {'map': torch.as_tensor(_DevArray(p[0].value, (N, S, S), '|i1'), device=dev),
                'agent_location': torch.as_tensor(_DevArray(p[1].value, (N, 2), '<i4'), device=dev),
                'agent_facing_id': torch.as_tensor(_DevArray(p[2].value, (N,), '<i4'), device=dev),
                'inventory_items_quantity': torch.as_tensor(_DevArray(p[3].value, (N, K), '<i4'), device=dev)}

    def device_outputs(self):
        import torch
        p = [C.c_void_p() for _ in range(3)]
        _cabi.check(_cabi.lib().ngw_out_device_ptrs(self._h, *[C.byref(x) for x in p]))
        N, dev = self.num_envs, 'cuda:%d' % self.device
        return {'reward': torch.as_tensor(_DevArray(p[0].value, (N,), '<i4'), device=dev),
                'done': torch.as_tensor(_DevArray(p[1].value, (N,), '|u1'), device=dev),
                'info': torch.as_tensor(_DevArray(p[2].value, (N,), '<i4'), device=dev)}

    # ------------------------------------------------------------------ action masks (include/ngw.h ngw_set_action_mask)
    @property
    def n_actions(self):
        """Actions of the handle's spec: the width of action_masks() (a novelty may add actions beyond action_space.n)."""
        return len(self.actions_id)

    def set_action_masks(self, on=True):
        """on: every step leaves the action masks of the state it produced behind it on the device (one more kernel launch per
        step); off: action_masks() computes them when asked.  Either way action_masks() describes the current state."""
        self._act_masks_on = bool(on)
        _cabi.check(_cabi.lib().ngw_set_action_mask(self._h, int(self._act_masks_on)))

    def action_mask_words(self, device=False, copy=False):
        """The packed masks of the current state: uint64 [N], bit a = step(a) would report info['result'] == True.  On the host this is the
        handle's ONE page-locked array, overwritten by the next call (copy=True: a fresh array); device=True: a torch int64 tensor over the
        handle's device buffer (zero copy, valid until the next call that changes the state)."""
        L = _cabi.lib()
        if device:
            import torch
            _cabi.check(L.ngw_action_mask(self._h))
            p = C.c_void_p()
            _cabi.check(L.ngw_action_mask_device_ptr(self._h, C.byref(p)))
            self.sync()
            return torch.as_tensor(_DevArray(p.value, (self.num_envs,), '<i8'), device='cuda:%d' % self.device)
        w = self.__dict__.get('_mask_words')
        if w is None:
            w = self._mask_words = _cabi.pinned_array((self.num_envs,), np.uint64)
        _cabi.check(L.ngw_get_action_mask(self._h, _cabi._ptr(w, np.uint64)))
        return w.copy() if copy else w

    def action_masks(self, device=False, copy=False):
        """Invalid-action masks of the current state (the state the next step() acts on): bool [N, n_actions], True where step(a) would
        report info['result'] == True.  device=True: a torch bool tensor on the handle's device, expanded from the packed words with torch
        ops.  The host array is a new array either way; `copy` is accepted for symmetry with the other observation calls."""
        if device:
            return unpack_action_masks_device(self.action_mask_words(device=True), self.n_actions)
        return unpack_action_masks(self.action_mask_words(), self.n_actions)

    # ------------------------------------------------------------------ one-step lookahead tables (include/ngw.h ngw_lookahead)
    def lookahead(self, device=False, copy=False):
        """Every action's outcome for every env, from the current state, without taking a step: a Lookahead of 'reward' int32 [N, A],
        'done' bool [N, A], 'result' bool [N, A] and 'info' uint32 [N, A] (the packed words: decode_info_words(info[:, a]) gives what
        step_costs() / messages() take).  Entry (i, a) is what step() would report for env i with action a, under every novelty and the
        autoreset setting; nothing is committed (no state byte changes, no reset runs, no prepared episode is consumed), and a second call
        without a change of state launches nothing.  On the host these are the handle's own arrays, overwritten by the next call
        (copy=True: fresh arrays).  device=True: zero-copy torch tensors shaped [N, A] over the device table - strided views of its
        action-major layout, valid until the next call that changes the state; 'info' is int32 there (the same bits), 'result' is
        computed from it."""
        L, N, A = _cabi.lib(), self.num_envs, self.n_actions
        if device:
            import torch
            _cabi.check(L.ngw_lookahead(self._h))
            p = [C.c_void_p() for _ in range(3)]
            es, as_ = C.c_int64(), C.c_int64()
            _cabi.check(L.ngw_lookahead_device_ptrs(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(es), C.byref(as_)))
            assert es.value == 1, "the device table is action-major"
            self.sync()
            dev = 'cuda:%d' % self.device
            view = lambda ptr, ts: torch.as_tensor(_DevArray(ptr.value, (A, as_.value), ts), device=dev)[:, :N].t()   # noqa: E731
            info = view(p[2], '<i4')
            return Lookahead(view(p[0], '<i4'), view(p[1], '|u1').view(torch.bool), (info & 1).bool(), info)
        h = self.__dict__.get('_look_host')
        if h is None or h[0].shape != (N, A):
            h = self._look_host = (np.zeros((N, A), np.int32), np.zeros((N, A), np.uint8), np.zeros((N, A), np.uint32))
        _cabi.check(L.ngw_get_lookahead(self._h, _cabi._ptr(h[0], np.int32), _cabi._ptr(h[1], np.uint8), _cabi._ptr(h[2], np.uint32)))
        reward, done, info = (x.copy() for x in h) if copy else h
        return Lookahead(reward, done.view(np.bool_), (info & 1).astype(np.bool_), info)

    # ------------------------------------------------------------------ plan evaluation (include/ngw.h ngw_plan_eval)
    def evaluate_plans(self, plans, device=False, copy=False):
        """What P candidate action sequences of T steps would return from the CURRENT state of every env, without committing a step: a
        PlanEval of 'ret' int32, 'length' int32, 'ended' bool and 'info' uint32, each [N, P].  Plan p of env i is stepped on a private copy
        by the rules step() applies (every novelty, the autoreset setting and horizon) and stops at the first step that ends the episode -
        that step counts; nothing is committed (no state byte changes, no reset runs, no prepared episode is consumed, masks and the
        lookahead table stay current).
        plans: an integer array [N, P, T], env-major, in host memory - validated here (an id outside the action list raises the ValueError
        step() raises and nothing launches) and transposed into a device staging buffer the env keeps; or a contiguous torch int32 tensor
        [T, P, N] on the env's device, used in place and unvalidated (an id outside the list is a no-op step of reward 0 that counts in
        'length' and raises the sticky NGW_F_INVALID_ACTION, see error_flags()).
        On the host the results are the env's own arrays, overwritten by the next call (copy=True: fresh arrays).  device=True: zero-copy
        torch tensors [N, P] over the plan-major device buffers, valid until the next evaluate_plans; 'info' is int32 there (the same bits)."""
        N = self.num_envs
        if hasattr(plans, 'data_ptr'):                          # a torch tensor on the device, [T, P, N]
            import torch
            assert plans.dtype == torch.int32 and plans.is_cuda and plans.is_contiguous(), "device plans: a contiguous torch int32 tensor on the GPU"
            assert plans.dim() == 3 and plans.shape[2] == N, "device plans are shaped [T, P, N]"
            assert plans.device.index == self.device, "device plans live on the env's device"
            T_, P = int(plans.shape[0]), int(plans.shape[1])
            self.evaluate_plans_ptr(plans.data_ptr(), N, P, T_)
        else:
            import torch
            a = np.asarray(plans)
            assert a.dtype.kind in 'iu', "plans are integer action ids"
            assert a.ndim == 3 and a.shape[0] == N, "host plans are shaped [N, P, T]"
            P, T_ = int(a.shape[1]), int(a.shape[2])
            A = len(self.actions_id)
            bad = (a < 0) | (a >= A)
            if bad.any():
                raise ValueError("%d is not in list" % int(a[bad][0]))
            tpn = np.ascontiguousarray(a.transpose(2, 1, 0), np.int32)
            stage = self.__dict__.get('_plan_stage')
            if stage is None or stage.numel() < tpn.size:
                stage = self._plan_stage = torch.empty(tpn.size, dtype=torch.int32, device='cuda:%d' % self.device)
            stage[:tpn.size].copy_(torch.from_numpy(tpn).reshape(-1))       # (from pageable memory: complete when it returns)
            torch.cuda.current_stream(self.device).synchronize()
            self.evaluate_plans_ptr(stage.data_ptr(), N, P, T_)
        L = _cabi.lib()
        if device:
            import torch
            p = [C.c_void_p() for _ in range(4)]
            es, ps = C.c_int64(), C.c_int64()
            _cabi.check(L.ngw_plan_eval_device_ptrs(self._h, *[C.byref(x) for x in p], C.byref(es), C.byref(ps)))
            assert es.value == 1, "the device results are plan-major"
            self.sync()
            dev = 'cuda:%d' % self.device
            view = lambda ptr, ts: torch.as_tensor(_DevArray(ptr.value, (P, ps.value), ts), device=dev)[:, :N].t()   # noqa: E731
            return PlanEval(view(p[0], '<i4'), view(p[1], '<i4'), view(p[2], '|u1').view(torch.bool), view(p[3], '<i4'))
        h = self.__dict__.get('_plan_host')
        if h is None or h[0].shape != (N, P):
            h = self._plan_host = (np.zeros((N, P), np.int32), np.zeros((N, P), np.int32), np.zeros((N, P), np.uint8), np.zeros((N, P), np.uint32))
        _cabi.check(L.ngw_get_plan_eval(self._h, _cabi._ptr(h[0], np.int32), _cabi._ptr(h[1], np.int32), _cabi._ptr(h[2], np.uint8),
                                        _cabi._ptr(h[3], np.uint32)))
        ret, length, ended, info = (x.copy() for x in h) if copy else h
        return PlanEval(ret, length, ended.view(np.bool_), info)

    def evaluate_plans_ptr(self, plans_ptr, env_stride, n_plans, n_steps):
        """The launch alone, for callers with their own memory (in the style of rollout_actions): the action of env i, plan p, step t is the
        int32 at device address plans_ptr + 4 * ((t * n_plans + p) * env_stride + i).  Enqueued on the env's stream; the results are read
        with ngw_get_plan_eval / ngw_plan_eval_device_ptrs (include/ngw.h)."""
        _cabi.check(_cabi.lib().ngw_plan_eval(self._h, C.c_void_p(int(plans_ptr)) if plans_ptr else None, int(env_stride), int(n_plans), int(n_steps)))

    # ------------------------------------------------------------------ multi-GPU observation stack (dist.py)
    def pack_layout(self):
        """Byte offsets of the seven payload sections + the payload size (include/ngw.h ngw_pack_layout)."""
        offs = (C.c_uint64 * 8)()
        _cabi.check(_cabi.lib().ngw_pack_layout(self._h, offs))
        return [int(x) for x in offs]

    def pack_obs(self, payload_ptr):
        """One launch: observation + step outputs -> the contiguous device payload at `payload_ptr` (16-byte aligned)."""
        _cabi.check(_cabi.lib().ngw_pack_obs(self._h, C.c_void_p(int(payload_ptr))))

    def unpack_obs(self, payloads_ptr, world, dst_ptrs):
        """Root side: `world` payloads back to back -> the global arrays at dst_ptrs (map, loc, facing, inv, reward, done, info)."""
        _cabi.check(_cabi.lib().ngw_unpack_obs(self._h, C.c_void_p(int(payloads_ptr)), int(world),
                                               *[C.c_void_p(int(x)) if x else None for x in dst_ptrs]))

    # ------------------------------------------------------------------ LidarInFront observation
    def lidar_configure(self, lidar_config=None, num_beams=8, fused=False, dtype=np.int16):
        """Enable the LidarInFront observation (reference observation_wrappers.py:10-80).  `lidar_config` fixes the lidar
        item set at wrap time like the reference wrapper does; by default it is built from the current spec.
        fused=True: every reset / step / rollout launch refreshes the observation in its own epilogue (no extra launch).
        dtype: the row format on the device and of what lidar_observation() returns - np.int16 (default: a beam entry is a
        range <= 64, inventory counts saturate at 32767), np.int32, or 'packed' (uint8 beam entries + int16 inventory tail,
        70 B per env for the reference's 8 beams; lidar_observation() then returns the pair (beams uint8 [N, B * NC],
        inventory int16 [N, NI]) as views of one buffer)."""
        from .lidar import LidarConfig
        self.lidar = lidar_config if lidar_config is not None else LidarConfig(self.spec, num_beams)
        self._lidar_c = self.lidar.compile(self.spec)
        L = _cabi.lib()
        self.lidar_refused = None
        try:
            _cabi.check(L.ngw_lidar_configure(self._h, C.byref(self._lidar_c)))
        except ValueError as e:
            self.lidar = None                                 # (not configured: nothing below ran)
            if ' B of LDS' in str(e):                         # the maps do not fit the observation's LDS layout: the handle cannot serve it
                from .snapshot import MapsTooLarge
                self.lidar_refused = str(e)
                raise MapsTooLarge(str(e)) from None
            raise
        self.lidar_len = self.lidar.obs_len(self.spec)
        self.lidar_packed = isinstance(dtype, str) and dtype == 'packed'
        self.lidar_dtype = np.dtype(np.uint8) if self.lidar_packed else np.dtype(dtype)
        assert self.lidar_packed or self.lidar_dtype in (np.dtype(np.int32), np.dtype(np.int16)), "lidar dtype must be int32, int16 or 'packed'"
        _cabi.check(L.ngw_lidar_set_output(self._h, 8 if self.lidar_packed else self.lidar_dtype.itemsize * 8))
        lay = [C.c_int32() for _ in range(4)]
        _cabi.check(L.ngw_lidar_row_layout(self._h, *[C.byref(x) for x in lay]))
        self.lidar_row_bytes, self._lidar_beam_bytes, self._lidar_inv_off, self._lidar_inv_bytes = [int(x.value) for x in lay]
        if self.lidar_packed:
            self._lidar_host = _cabi.pinned_array((self.num_envs, self.lidar_row_bytes), np.uint8)
        else:
            self._lidar_host = _cabi.pinned_array((self.num_envs, self.lidar_len), self.lidar_dtype)
        self.lidar_fused = bool(fused)
        _cabi.check(L.ngw_lidar_fuse(self._h, int(self.lidar_fused)))
        # fused: the packed host step of a big batch brings the rows of the state it produced across with its own slices (one call, one
        # synchronisation): lidar_observation() then hands out this buffer as long as nothing else has stepped the env since
        self._lidar_rows_fresh = False
        if self.lidar_fused and hasattr(L, 'ngw_lidar_host_rows'):
            _cabi.check(L.ngw_lidar_host_rows(self._h, _cabi._ptr(self._lidar_host, self.lidar_dtype)))

    def _lidar_split(self, rows):
        """(beams uint8 [N, B * NC], inventory int16 [N, NI]) views of packed rows (numpy array or torch tensor [N, row_bytes])."""
        nb = self.lidar.num_beams * len(self.lidar.lidar_items_id)
        beams, tail = rows[:, :nb], rows[:, self._lidar_inv_off:]
        if isinstance(rows, np.ndarray):
            return beams, tail.view(np.int16)
        import torch
        return beams, tail.view(torch.int16)

    def lidar_observation(self, device=False, copy=False):
        """[N, num_beams * n_lidar_items + n_inventory] observation of the current state in the configured dtype (one kernel
        launch, or none in fused mode - then it is the observation the last reset / step / rollout launch produced); with the
        packed format the pair (beams, inventory), see lidar_configure."""
        if not self.lidar_fused:
            _cabi.check(_cabi.lib().ngw_lidar(self._h))
        elif not device and self.__dict__.get('_lidar_rows_fresh'):   # the last call was a packed host step: it delivered the rows already
            out = self._lidar_host.copy() if copy else self._lidar_host
            return self._lidar_split(out) if self.lidar_packed else out
        if device:
            import torch
            p = C.c_void_p()
            _cabi.check(_cabi.lib().ngw_lidar_device_ptr(self._h, C.byref(p)))
            self.sync()
            if self.lidar_packed:
                raw = torch.as_tensor(_DevArray(p.value, (self.num_envs, self.lidar_row_bytes), '|u1'), device='cuda:%d' % self.device)
                return self._lidar_split(raw)
            return torch.as_tensor(_DevArray(p.value, (self.num_envs, self.lidar_len), self.lidar_dtype.str), device='cuda:%d' % self.device)
        _cabi.check(_cabi.lib().ngw_get_lidar(self._h, _cabi._ptr(self._lidar_host, self.lidar_dtype)))
        out = self._lidar_host.copy() if copy else self._lidar_host
        return self._lidar_split(out) if self.lidar_packed else out

    def lidar_widen(self, packed_pair, dtype=np.int32):
        """The [N, L] array of `dtype` from a packed (beams, inventory) pair (host side)."""
        beams, tail = packed_pair
        out = np.empty((beams.shape[0], beams.shape[1] + tail.shape[1]), dtype)
        out[:, :beams.shape[1]] = beams
        out[:, beams.shape[1]:] = tail
        return out

    # ------------------------------------------------------------------ state (checkpoint / oracle injection)
    def get_state(self, first=0, count=None):
        count = self.num_envs - first if count is None else count
        S2, K = self.map_size ** 2, self.n_items
        st = {'map': np.zeros((count, S2), np.int8), 'loc': np.zeros((count, 2), np.int32),
              'facing': np.zeros(count, np.int32), 'inv': np.zeros((count, K), np.int32),
              'selected': np.zeros(count, np.int32), 'step_count': np.zeros(count, np.int32),
              'episode': np.zeros(count, np.uint32)}
        _cabi.check(_cabi.lib().ngw_get_state(self._h, first, count, _cabi._ptr(st['map'], np.int8), _cabi._ptr(st['loc'], np.int32),
                                              _cabi._ptr(st['facing'], np.int32), _cabi._ptr(st['inv'], np.int32),
                                              _cabi._ptr(st['selected'], np.int32), _cabi._ptr(st['step_count'], np.int32),
                                              _cabi._ptr(st['episode'], np.uint32)))
        return st

    def set_state(self, first=0, map=None, loc=None, facing=None, inv=None, selected=None, step_count=None, episode=None):
        self._lidar_rows_fresh = False
        arrs = [(map, np.int8), (loc, np.int32), (facing, np.int32), (inv, np.int32), (selected, np.int32),
                (step_count, np.int32), (episode, np.uint32)]
        conv = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in arrs]
        counts = {len(a) for a in conv if a is not None}
        assert len(counts) == 1, "all state arrays must cover the same number of envs"
        count = counts.pop()
        if conv[0] is not None:
            conv[0] = conv[0].reshape(count, -1)
        _cabi.check(_cabi.lib().ngw_set_state(self._h, first, count, *[_cabi._ptr(a, dt) for a, (_, dt) in zip(conv, arrs)]))

    # ------------------------------------------------------------------ device-side snapshots (snapshot.py, include/ngw.h ngw_snapshot_*)
    def snapshot(self, capacity=None):
        """A buffer of `capacity` saved env states on the device (default: one slot per env): Snapshot.save / restore / state / close.
        It belongs to this env and is closed with it, and by an in-place rebuild() (inject_novelty)."""
        from .snapshot import Snapshot
        s = Snapshot(self, self.num_envs if capacity is None else capacity)
        self.__dict__.setdefault('_snapshots', []).append(s)
        return s

    def state_keys(self, envs=None, fields=KEY_STATE, device=False):
        """The 64-bit state keys of the envs' CURRENT states: numpy uint64 [count], entry j the key of env envs[j] (None: every env; a list /
        numpy array, checked, may repeat; or a torch int32 tensor on the env's device, used in place: an index out of range gives key 0 and
        raises F_BAD_INDEX) under the field selection `fields` (KEY_* bits) - Snapshot.keys() without the save: the key of an env equals the
        key of a slot that holds its state.  One kernel launch; nothing is committed (masks, lookahead table, lidar rows and prepared
        episodes stay current).  device=True: a torch int64 tensor over the same bits, ordered behind the launch on torch's current
        stream, no host wait."""
        import torch
        from .snapshot import enqueue_ordered, index_arg
        f = check_fields(fields)
        ptr, count, dev, uploaded = index_arg(self, envs, self.num_envs, 'envs')
        words = torch.empty(count, dtype=torch.int64, device=dev)
        enqueue_ordered(self, self._keeper(), lambda: _cabi.lib().ngw_state_keys(self._h, None, ptr, count, f, C.c_void_p(words.data_ptr())), count, uploaded,
                        device)
        return words if device else words.cpu().numpy().view(np.uint64)

    # ------------------------------------------------------------------ device-side key tables (key_table.py, include/ngw.h ngw_key_table_*)
    def key_table(self, capacity, values=False, **kw):
        """A hash set of 64-bit keys on the device with room for `capacity` of them: KeyTable.insert / lookup / clear / close, len().  It
        answers "have I seen this state before?" across calls, where Snapshot.unique() groups equal states within one call.  values=True:
        the table also keeps the smallest int32 value offered with each key and a tag beside it - KeyTable.insert_min / read / get /
        trace: "is this the cheapest way I have found to this state, and which way was it?"; a table without values costs what it always
        cost.  It belongs to this env and is closed with it, and by an in-place rebuild() (inject_novelty)."""
        from .key_table import KeyTable
        t = KeyTable(self, capacity, values, **kw)
        self.__dict__.setdefault('_key_tables', []).append(t)
        return t

    def insert_state_keys(self, table, envs=None, fields=KEY_STATE, device=False):
        """state_keys(envs, fields) offered to `table` (a KeyTable of this env): (keys, KeyInsert(where, fresh)) - Snapshot.insert_keys() for
        the envs' CURRENT states; the keys stay on the device between the two calls."""
        table._open_for(self)
        keys = self.state_keys(envs, fields, device=True)
        found = table.insert(keys, device=device)
        return (keys if device else keys.cpu().numpy().view(np.uint64)), found

    def insert_state_keys_min(self, table, values, tags=None, envs=None, fields=KEY_STATE, device=False):
        """state_keys(envs, fields) offered to `table` (a KeyTable of this env made with values=True) with `values` and `tags`: (keys,
        KeyBest(where, fresh, best)) - Snapshot.insert_keys_min() for the envs' CURRENT states; the keys stay on the device between the two
        calls."""
        table._open_for(self)
        keys = self.state_keys(envs, fields, device=True)
        found = table.insert_min(keys, values, tags, device=device)
        return (keys if device else keys.cpu().numpy().view(np.uint64)), found

    def _keeper(self):
        keeper = self.__dict__.get('_keys_keeper')
        if keeper is None:
            keeper = self._keys_keeper = _Keeper()
        return keeper

    def successor_keys(self, envs=None, fields=KEY_STATE, device=False, reports=True):
        """The key of every action's child of the envs' CURRENT states, with no child stored: Snapshot.successor_keys() without the save - a
        SuccessorKeys of [count, A] fields, keys[j, a] the key of the state step(a) would leave env envs[j] in before any reset, reward / done
        / result / info [j, a] what lookahead() reports for it.  envs as in state_keys().  One kernel launch; nothing is committed."""
        from .snapshot import successor_keys_call
        return successor_keys_call(self, self._keeper(), None, envs, self.num_envs, 'envs', fields, device, reports)

    def walk_distances(self, envs=None, device=False):
        """How far the envs' agents are from facing each item in their CURRENT states: int32 [count, K] - Snapshot.walk_distances() without
        the save (the contract: include/ngw.h ngw_snapshot_walk, walk.shortest_walk on the host).  envs as in state_keys() (an index out of
        range in a device list: a row of -1, F_BAD_INDEX).  One kernel launch; nothing is committed."""
        from .walk import walk_call
        return walk_call(self, self._keeper(), None, envs, self.num_envs, 'envs', None, 0, device, want_plans=False)

    def recipe_costs(self, envs=None, costs=None, scale=1, device=False):
        """What the envs' CURRENT states still have to pay in crafts, extractions and breaks before they hold the goal item, at the least:
        int32 [count] - Snapshot.recipe_costs() without the save (the contract: include/ngw.h ngw_snapshot_recipe_costs,
        search.recipe_cost_reference on the host).  costs / scale as Snapshot.search takes them; envs as in state_keys() (an index out of range
        in a device list: 0, F_BAD_INDEX).  One kernel launch; nothing is committed."""
        from .search import recipe_call
        return recipe_call(self, self._keeper(), None, envs, self.num_envs, 'envs', costs, scale, device)

    def walk_plans(self, items, steps, envs=None, device=False):
        """The shortest walk of each env's agent from its CURRENT state to the nearest cell of items[j], as a plan: Snapshot.walk_plans()
        without the save - WalkPlans(plans [steps, count], length [count], dist [count, K]).  items, steps and device as there, envs as in
        state_keys().  One kernel launch; nothing is committed."""
        from .walk import walk_call
        return walk_call(self, self._keeper(), None, envs, self.num_envs, 'envs', items, steps, device)

    def insert_successor_keys(self, table, envs=None, fields=KEY_STATE, device=False):
        """successor_keys(envs, fields) offered to `table` (a KeyTable of this env): Snapshot.insert_successor_keys() for the envs' CURRENT
        states."""
        from .snapshot import insert_successors
        table._open_for(self)
        return insert_successors(self.successor_keys(envs, fields, device=True), table, device)

    def sample_actions(self, weights, seed, t=0, envs=None, device=False):
        """One action per env, drawn with probability proportional to the caller's weights among the actions the env's CURRENT state accepts
        (every action where it accepts none) - invalid-action masking, the normalisation and the draw of a policy-gradient loop in one
        kernel launch.  weights: a host array [count, A] of non-negative numbers (checked for shape and dtype, transposed and uploaded), or
        a torch float32 tensor [A, count] on the env's device - action-major - that is used in place.  Returns Sampled(action int32, mass
        float32, mask_words uint64), each [count]: mass is the sum of the valid actions' weights, so log pi(a) = log weights[a] - log mass
        (0 where no valid action had a weight and the choice was uniform among the valid ones); mask_words is the valid-action word the
        choice was made under.  The choice is the public contract of include/ngw.h (ngw_sample_actions), which sample.choose_weighted
        computes on the host bit for bit: it depends on (seed, env_index_base + j, t), the state and the weights alone, so the ranks of a
        sharded env return what one unsharded env returns; pass a new t (or seed) for every step of a trajectory.  A weight below 2^-64
        counts as 0; a negative, NaN or larger-than-2^64 weight counts as 0 too and raises the sticky F_BAD_WEIGHT (error_flags()), from the
        host and from the device alike.  envs as in state_keys() (an index out of range in a device list: action -1, mass 0, word 0,
        F_BAD_INDEX).  Nothing is committed.  device=True: torch tensors on the env's device (the words int64 over the same bits), ordered
        behind the launch on torch's current stream, no host wait."""
        from .sample import sample_call
        return sample_call(self, self._keeper(), None, envs, self.num_envs, 'envs', weights, seed, self.env_index_base, t, device)

    def step_sampled(self, weights, seed, t=0):
        """sample_actions(weights, seed, t, device=True) followed by step_device on the sampled actions: two launches on the env's stream with
        no host wait in between.  Returns the Sampled tuple on the device - the actions the step took, the mass and the mask words of the
        state BEFORE the step; the step's outputs are where step_device leaves them (device_outputs())."""
        s = self.sample_actions(weights, seed, t, device=True)
        self._keeper()._keep = (self._keeper()._keep or []) + [s.action]     # (the step reads the tensor after this call returns)
        self.step_device(s.action.data_ptr())
        return s

    def playouts(self, n_playouts, steps, seed, device=False, weights=None, path_keys=False, fields=None, rewards=False, masks=False, observe=None,
                 view_size=5, table=None, table_weights=None, outside='default'):
        """P = n_playouts valid-action random playouts of up to `steps` steps from every env's CURRENT state, without taking a step and
        without a snapshot of the caller's: Snapshot.playout(from_envs=True) with the parents repeat(arange(N), P).  Returns a Playout whose
        fields are [N, P] ('actions' is None: Snapshot.playout records them).  Playout q of env i is pair (env_index_base + i) * P + q of the
        stream of `seed` (the contract of include/ngw.h; playout.choose_actions on the host), so the ranks of a sharded env return what one
        unsharded env returns.  One kernel launch; nothing is committed.  device=True: torch tensors on the env's device, ordered behind
        the launch on torch's current stream.  weights: float32 [A] (host or device) - every step's action is then drawn with probability
        proportional to them among the valid ones (Snapshot.playout).  path_keys=True: a PlayoutPath whose 'keys' [T, N, P] hold the key
        under `fields` (default KEY_STATE) of the state every playout is in after each executed step, 0 for the others (Snapshot.playout).
        rewards=True / masks=True / observe='lidar': a PlayoutTraj with 'rewards' [T, N, P], 'masks' [T, N, P] and 'obs' [T + 1, N, P, row] - every
        step's reward, the mask word its choice was made under and the LidarInFront rows before and after it (Snapshot.playout; obs takes
        (T + 1) * N * P rows of device memory).  observe='agent_view' (view_size=V, default 5): 'obs' is the AgentMap dict of Snapshot.playout,
        'agent_map' [T + 1, N, P, W, W], 'agent_facing_id' [T + 1, N, P], 'inventory_items_quantity' [T + 1, N, P, K]; no lidar needed.
        table / table_weights / outside: a guided playout (Snapshot.playout) - a PlayoutGuided with 'where' [T, N, P] and 'depth' [N, P]."""
        import torch
        from .playout import check_guide
        from .snapshot import check_observe, check_playout, pairs_call
        P = int(n_playouts)
        if P < 1:
            raise ValueError("n_playouts: at least one playout per env expected, got %d" % P)
        N = self.num_envs
        dev = torch.device('cuda:%d' % self.device)
        parents = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(P).contiguous()
        _, _, count, steps = check_playout(parents, steps, None, N, 0, False, lambda x: None if x is None else int(x.numel()))
        check_observe(self, observe, view_size)
        guide = check_guide(self, table, table_weights, outside, fields)
        return pairs_call(self, self._keeper(), 'playout', None, None, parents, None, count, steps, device, seed=seed, first_pair=self.env_index_base * P,
                          weights=weights, path_keys=path_keys, fields=fields, rewards=rewards, masks=masks, observe=observe,
                          view_size=view_size, table=table, table_weights=table_weights, guide=guide).shaped(N, P)

    def fork(self, src, keep_episode=False):
        """Every env e becomes a copy of env src[e] (src: num_envs indices - a list / numpy array, checked, or a torch int32 tensor on the
        env's device), through an internal scratch snapshot: all states are saved first, so src may name any env, itself included.  The
        copies share the rest of the current episode and differ from their next reset on (each env draws from its own stream)."""
        if len(src) != self.num_envs:
            raise ValueError("fork: src names %d envs, the batch has %d" % (len(src), self.num_envs))
        s = self.__dict__.get('_fork_snap')
        if s is None or s.closed:
            s = self._fork_snap = self.snapshot()
        s.save()
        s.restore(slots=src, keep_episode=keep_episode)

    def _drop_snapshots(self, sync=True):
        """The handle is going: its snapshots' and key tables' buffers go with it (ngw_destroy), the Python objects raise from now on."""
        snaps = list(self.__dict__.get('_snapshots', ())) + list(self.__dict__.get('_key_tables', ()))
        if sync and self._h and any(s._keep for s in snaps):
            self.sync()                                       # (a queued save / restore may still be reading its uploaded index lists)
        for s in snaps:
            s._invalidate()
        self.__dict__['_snapshots'] = []
        self.__dict__['_key_tables'] = []
        self.__dict__.pop('_fork_snap', None)

    # ------------------------------------------------------------------ timing (bench roofline leg) / hipGraph stepping
    def timing_begin(self):
        _cabi.check(_cabi.lib().ngw_timing_begin(self._h))

    def timing_end(self):
        """Device milliseconds between timing_begin() and now on the handle's stream (HIP event pair)."""
        ms = C.c_double(0)
        _cabi.check(_cabi.lib().ngw_timing_end(self._h, C.byref(ms)))
        return ms.value

    def graph_build(self, actions_ptr, step_stride, n_steps):
        """Capture n_steps step_device launches reading actions_ptr + i * step_stride (int32 elements) into one hipGraph."""
        _cabi.check(_cabi.lib().ngw_graph_build(self._h, C.c_void_p(int(actions_ptr)), int(step_stride), int(n_steps)))

    def graph_launch(self, reps=1):
        self._lidar_rows_fresh = False
        _cabi.check(_cabi.lib().ngw_graph_launch(self._h, int(reps)))

    def timing_mark(self):
        """Record the closing event of the timing pair without waiting for it (timing_end then only reads the pair)."""
        _cabi.check(_cabi.lib().ngw_timing_mark(self._h))

    def set_agent_view(self, view_size=5, fused=True):
        """Keep the AgentMap window current (include/ngw.h ngw_agent_view_fuse): after it, every committed step and every reset - step,
        step_device, step_device_many, a replayed graph, step_sampled, rollout, reset with or without a mask - leaves the int8 [N, W, W] windows
        (W = 2 * view_size + 1) of the state it produced in the handle's view buffer, on the handle's stream: what agent_view(view_size) called right
        after it returns, byte for byte, with no second call and no host wait.  fused=True: the in-place step kernel builds the windows in the
        launch that steps, where it fuses nothing else (no fused lidar, no action masks, no host write-through, and view_size <= 2 - larger windows measured slower than the
        second launch); every other
        launch is followed by the stand-alone gather.  fused=False: the gather behind every launch (the A/B form).  set_agent_view(None) switches
        it off.  A graph is built after this call, not before."""
        if view_size is None:
            _cabi.check(_cabi.lib().ngw_agent_view_fuse(self._h, 0, 0))
            self._agent_view_cfg = None
            return
        V = check_view_size(view_size)
        _cabi.check(_cabi.lib().ngw_agent_view_fuse(self._h, V, 1 if fused else 2))
        self._agent_view_cfg = (V, bool(fused))                 # (rebuild() switches it on again on the new handle)

    def agent_view_observation(self, view_size=5, device=False, copy=False):
        """The AgentMap observation of the current state, the dict Snapshot.agent_view returns: 'agent_map' (agent_view's window), 'agent_facing_id'
        int32 [N] and 'inventory_items_quantity' int32 [N, K] - the last two are the env's own state arrays (device=True: zero-copy views of them),
        not the output of another kernel."""
        view = self.agent_view(view_size, device=device, copy=copy)
        if device:
            o = self.device_observation()
        else:
            o = self.get_observation(copy)
        return {'agent_map': view, 'agent_facing_id': o['agent_facing_id'], 'inventory_items_quantity': o['inventory_items_quantity']}

    def agent_view(self, view_size=5, device=False, copy=False):
        """AgentMap window (reference observation_wrappers.py:104-121): int8 [N, 2*view_size+1, 2*view_size+1], the map
        around each agent with 0 outside the map; one gather launch on the current state.  With set_agent_view(view_size) on, the windows of
        that size are kept current by the steps themselves: the call launches nothing unless the state was written some other way since
        (set_state, a snapshot restore), and device=True is the same buffer every time.  Another size is gathered into a buffer of its own."""
        _cabi.check(_cabi.lib().ngw_agent_view(self._h, int(view_size)))
        W = 2 * int(view_size) + 1
        if device:
            import torch
            p = C.c_void_p()
            _cabi.check(_cabi.lib().ngw_agent_view_device_ptr(self._h, C.byref(p)))
            self.sync()                                           # (the gather ran on the handle's stream, torch reads on its own)
            return torch.as_tensor(_DevArray(p.value, (self.num_envs, W, W), '|i1'), device='cuda:%d' % self.device)
        host = getattr(self, '_view_host', None)
        if host is None or host.shape[1] != W:
            host = self._view_host = np.zeros((self.num_envs, W, W), np.int8)
        _cabi.check(_cabi.lib().ngw_get_agent_view(self._h, _cabi._ptr(host, np.int8)))
        return host.copy() if copy else host
