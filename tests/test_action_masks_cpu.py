"""Action masks, host side (no GPU): the C-ABI surface, the Python surface, the unpacking and LimitActions column mapping on hand-built
words, and the oracle helper the GPU tests compare against, tied to the reference's recorded single-step outcomes (G4)."""
import os
import re

import numpy as np
import pytest

import mask_oracle as M
import ngw_testlib as T
from gym_novel_gridworlds_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_API = ['ngw_set_action_mask', 'ngw_action_mask', 'ngw_get_action_mask', 'ngw_action_mask_device_ptr']


def test_header_declares_and_library_exports_the_mask_api():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    L = _cabi.lib()
    for name in MASK_API:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert hasattr(L, name), name
        assert name in _cabi.SYMBOLS
    assert hasattr(L, 'ngw_debug_solo_starts')
    assert L.ngw_abi_version() == 3


def test_python_surface_has_the_mask_methods():
    from gym_novel_gridworlds_amd import LidarInFront, LimitActions, VecNovelGridworld
    from gym_novel_gridworlds_amd.dist import ShardedVecNovelGridworld
    from gym_novel_gridworlds_amd.envs import _NovelGridworldEnv
    from gym_novel_gridworlds_amd.novelty_wrappers import NoveltyWrapper
    from gym_novel_gridworlds_amd.observation_wrappers import AgentMap
    for cls, names in ((VecNovelGridworld, ('set_action_masks', 'action_masks', 'action_mask_words')),
                       (ShardedVecNovelGridworld, ('set_action_masks', 'action_masks', 'action_mask_words')),
                       (_NovelGridworldEnv, ('action_masks',)), (NoveltyWrapper, ('action_masks',)),
                       (LimitActions, ('action_masks',)), (LidarInFront, ('action_masks',)), (AgentMap, ('action_masks',))):
        for name in names:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    assert LimitActions.action_masks is not NoveltyWrapper.action_masks      # (it maps columns into its own id space)


def test_unpack_packed_words():
    from gym_novel_gridworlds_amd.vec_env import unpack_action_masks
    rs = np.random.RandomState(3)
    bits = rs.randint(0, 2, size=(37, 48)).astype(bool)
    words = np.zeros(37, np.uint64)
    for a in range(48):
        words |= bits[:, a].astype(np.uint64) << np.uint64(a)
    for A in (1, 9, 17, 48):
        got = unpack_action_masks(words, A)
        assert got.dtype == np.bool_ and got.shape == (37, A)
        assert (got == bits[:, :A]).all()
    assert (unpack_action_masks(np.array([1 << 63], np.uint64), 48) == False).all()   # bits >= n_actions are not columns  # noqa: E712


def test_limit_actions_column_mapping():
    from gym_novel_gridworlds_amd.wrappers import limit_mask_columns
    actions_id = {'Forward': 0, 'Left': 1, 'Right': 2, 'Break': 3, 'Craft_plank': 7}
    limited = dict(zip(sorted(['Break', 'Forward', 'Craft_plank', 'Nope']), range(4)))   # Break 0, Craft_plank 1, Forward 2, Nope 3
    inner = np.zeros((2, 8), bool)
    inner[0, [0, 3]] = True
    inner[1, [7, 2]] = True
    got = limit_mask_columns(inner, limited, actions_id, 4)
    assert got.tolist() == [[True, False, True, False], [False, True, False, False]]
    # the FIRST name holding a limited id (table order) decides, as in LimitActions.step
    got = limit_mask_columns(inner[0], {'Left': 0, 'Forward': 0}, actions_id, 1)
    assert got.tolist() == [False]


CFG_G4 = sorted(T.spec_json()['cfgs'])


def test_every_fixture_config_has_single_step_cases():
    assert len(CFG_G4) == 59
    for cfg in CFG_G4:
        assert len(T.golden(cfg)['ss_action']) > 0, cfg


@pytest.mark.parametrize('cfg', CFG_G4)
def test_oracle_mask_helper_agrees_with_reference_single_steps(cfg):
    """The helper's bit ss_action of every G4 pre-state is the reference's recorded ss_result."""
    g = T.golden(cfg)
    spec = T.build_spec(cfg)
    st = M.state_from(spec, g['ss_pre_map'], g['ss_pre_loc'], g['ss_pre_facing'], g['ss_pre_inv'], g['ss_pre_sel'])
    words = M.oracle_mask_words(spec, st)
    bit = (words >> g['ss_action'].astype(np.uint64)) & np.uint64(1)
    assert (bit == g['ss_result'].astype(np.uint64)).all()
    assert (words >> np.uint64(spec.compile().n_actions) == 0).all()
