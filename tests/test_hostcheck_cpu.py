"""The C-ABI's host side (gym_novel_gridworlds_amd/csrc/ngw_abi_*.cpp, ngw_host.h) under AddressSanitizer and UndefinedBehaviorSanitizer, with no GPU:
tests/hostcheck builds the unchanged host units against a fake HIP runtime (device memory = exact-size heap blocks, a ledger of what is alive)
and one stub per kernel launcher that touches every array over its documented extent.  Each scenario of tests/hostcheck/main.cpp runs as a
stand-alone program (the sanitizer runtimes are linked in; nothing is preloaded) and must exit 0; the -DFAKE_HIP_SHORT=8 build, which hands
allocations out 8 bytes short, and the leak scenario must NOT - the harness's proof that it can fail.  The harness says nothing about what a
kernel computes.

Specs: Pogostick-v1 at 9 x 9 and 10 x 10 (make_spec), and the committed configurations of tests/ngw_testlib.py by n_items (K) mod 4 - the
realignment of an open-list search's slab depends on it:
    K = 9  (K % 4 == 1)  pogo9, pogo10 (plain Pogostick-v1)
    K = 10 (K % 4 == 2)  axe10
    K = 11 (K % 4 == 3)  stk_add_repl12
    K = 12 (K % 4 == 0)  no entry of CFGS has 8 or 12 items (every one compiles to 9, 10 or 11), so the fixture stacks three committed
                         novelties on Bow-v1 at 12 x 12: additem/easy/arrow, axe/easy/wooden, fence/easy/oak.  This is the residue at which the
                         weights and the distances lie back to back in the slab, with no padding between them.
Pogostick-v1 at 36 x 36 is the second spec of `refusals`: maps that ngw_successor_keys and the searches refuse (more LDS than a CU has).  A tree
search is still made there - its guided playout keeps one set of maps, not two -, so the third spec, 48 x 48, is the one ngw_tree_create refuses:
by its closing call of no pairs, after the slab exists.

Measured where this was written (8 cores): building both programs 4.5 s; the slowest scenarios are `tree` and `search` over the five specs, 0.5 s
and 0.3 s; every other one is under 0.1 s.
"""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ngw_testlib as T  # noqa: E402
from gym_novel_gridworlds_amd.novelty import apply_novelty  # noqa: E402
from gym_novel_gridworlds_amd.spec import make_spec  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hostcheck')
BUILD = os.path.join(HERE, '_build')
TIMEOUT = 120

# FAKE_HIP_SHORT=8: the allocations whose last array ends within 8 bytes of the allocation's end - handing them out short must end in an
# AddressSanitizer report (scenario, allocation)
MUST_TRIP = [
    ('search', 'search_slab_closed'),    # ngw_search_create: ends with best[n], at most 7 bytes of tail slack
    ('search', 'search_slab_open'),      # ngw_search_create_open with the walk heuristic: likewise
    ('table', 'table_slab_plain'),       # ngw_key_table_create: ends with the counter of stored keys
    ('table', 'table_slab_valued'),      # ngw_key_table_create_valued: ends with tag[buckets]
    ('snapshot', 'snapshot_slab'),       # ngw_snapshot_create(64): episode[64] = 256 bytes, no padding behind it
    ('frontier', 'frontier_scratch_regrown'),   # regrown for 513 * 4096 + 1 flags: the ticket + 514 tile counts, exactly
    ('frontier', 'select_scratch_regrown'),     # regrown for 4 groups of 1025: NGW_SELECT_SCRATCH_WORDS(4, 1) = 4140 words, exactly
    ('tree', 'tree_slab'),               # ngw_tree_create: ends with ended[P], fresh[P] inside (2 P + 7) / 8 words, at most 7 bytes of tail slack
    ('recipe', 'search_recipe_term'),    # ngw_search_set_recipe on a search of capacity 3: [cap] int32, exactly
]
# the size each picked allocation is asked for (9 items, 17 actions, 10 x 10; the fake prints it): the proof that the name picks what it says
PICKED_BYTES = {'frontier_scratch': 513 * 4, 'select_scratch': 4096 * 4, 'frontier_scratch_regrown': 515 * 4, 'select_scratch_regrown': 4140 * 4,
                'table_slab_plain': (2 * 2 + 1) * 8, 'table_slab_valued': (2 * 2 + 1 + 2 + 1) * 8, 'snapshot_slab': 64 * 100 + 64 * 9 * 4 + 512 + 4 * 256,
                'snapshot_slab_padded': 6656 + 2560 + 768 + 512 + 256 + 512 + 512,
                # 2 + n 64-bit words, 332 + 6 cap + 2 pool + 4 n int32 (n = cap * 17 = 17, pool 64), 2 n flag bytes rounded up to 8
                'search_slab_closed': (2 + 17) * 8 + (332 + 6 + 128 + 68) * 4 + 40,
                # P = 1 playout of T = 1 step, a table of capacity 64 (128 buckets), 17 actions, no priors (include/ngw.h, ngw_tree_device_arrays; ngw_host.h):
                # 64-bit words: returns 128 * 17, mask_words 128, keys and masks T * P each, leaf_keys and leaf_masks P each;
                # 32-bit words: visits and rows 128 * 17 each, actions / rewards / where / touched T * P each, the eight [P] arrays (depth, length, ret,
                #   first_action, where_leaf, roots, start_actions, info), the zero weight block 17 * P, the weights 17 -> 18, the stats ring 65 * 8 - 4919, made even;
                # ended[P] and fresh[P] in one 64-bit word
                'tree_slab': (128 * 17 + 128 + 2 + 2) * 8 + (2 * 128 * 17 + 4 + 8 + 17 + 18 + 65 * 8 + 1) * 4 + 8,
                'search_recipe_term': 3 * 4}
# ... and the ones the product rounds up on purpose: short by 8 bytes they still hold everything a launch may touch (scenario, allocation, the rule)
ROUNDED_UP = [
    ('frontier', 'select_scratch', 'ngw_frontier_select: at least 4096 words; the calls before the first regrow use at most 1044'),
    ('frontier', 'frontier_scratch', 'ngw_frontier_compact: the ticket + at least 512 tile counts; the calls before the first regrow use 3 words'),
    ('snapshot', 'snapshot_slab_padded', 'ngw_snapshot_create(65): every array padded to 256 bytes, episode[65] leaves 252 behind it'),
]
SCENARIOS = ['handle', 'host_step', 'snapshot', 'table', 'frontier', 'search', 'tree', 'recipe', 'refusals']
# what a scenario must have reached (stub name -> at least one call), read from the stubs' own counters
MUST_REACH = {
    'host_step': ['ngw_launch:wire', 'ngw_launch:lidar', 'ngw_launch:refill', 'mirror_out', 'ngw_pack_launch', 'ngw_diff_launch', 'ngw_wire_launch',
                  'ngw_diff_wire_launch'],
    'search': ['ngw_search_take_launch', 'ngw_search_open_launch', 'ngw_search_offer_launch', 'ngw_search_judge_launch', 'ngw_search_settle_launch',
               'ngw_search_roots_launch', 'ngw_walk_launch', 'ngw_frontier_select_launch', 'ngw_frontier_compact_launch', 'ngw_frontier_alloc_launch',
               'ngw_successors_launch', 'ngw_expand_launch', 'ngw_table_insert_min_launch', 'ngw_table_read_launch', 'ngw_keys_launch'],
    'table': ['ngw_table_insert_launch', 'ngw_table_lookup_launch', 'ngw_table_insert_min_launch', 'ngw_table_read_launch', 'ngw_table_trace_launch',
              'ngw_table_renorm_launch'],
    'snapshot': ['ngw_snapshot_launch', 'ngw_expand_launch', 'ngw_keys_launch', 'ngw_successors_launch', 'ngw_walk_launch', 'ngw_slot_mask_launch'],
    'frontier': ['ngw_frontier_compact_launch', 'ngw_frontier_alloc_launch', 'ngw_frontier_select_launch'],
    'tree': ['ngw_tree_leaf_launch', 'ngw_tree_grow_launch', 'ngw_tree_backup_launch', 'ngw_tree_backup_discount_launch', 'ngw_tree_reweight_launch',
             'ngw_tree_reweight16_launch', 'ngw_playout_guided_launch', 'ngw_table_insert_launch', 'ngw_keys_launch', 'ngw_sample_launch'],
    'recipe': ['ngw_recipe_launch', 'ngw_search_open_launch', 'ngw_search_roots_launch'],
}


def _sanitizers_work(tmp):
    """g++ links and runs a one-line -fsanitize=address,undefined program: the only reason this module may skip."""
    if not shutil.which('g++'):
        return False, 'g++ not found'
    src = os.path.join(tmp, 'one.cpp')
    with open(src, 'w') as f:
        f.write('int main() { return 0; }\n')
    exe = os.path.join(tmp, 'one')
    r = subprocess.run(['g++', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe, src], capture_output=True, text=True)
    if r.returncode:
        return False, 'g++ -fsanitize=address,undefined does not link: ' + r.stderr[-300:]
    r = subprocess.run([exe], capture_output=True, text=True)
    if r.returncode:
        return False, 'a sanitized program does not run here: ' + r.stderr[-300:]
    return True, ''


def _env():
    env = {k: v for k, v in os.environ.items() if not k.startswith('NGW_')}      # (the product's switches: the scenarios set their own)
    env['HOSTCHECK_STUB_COUNTS'] = '1'
    return env


@pytest.fixture(scope='session')
def hostcheck(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('hostcheck'))
    ok, why = _sanitizers_work(tmp)
    if not ok:
        print('test_hostcheck_cpu skipped: ' + why)
        pytest.skip(why)
    r = subprocess.run(['make', '-C', HERE, 'hostcheck', 'hostcheck_short'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    specs = []
    k12 = make_spec(T.BOW, 12)
    for one in (('additem', 'easy', 'arrow', ''), ('axe', 'easy', 'wooden', ''), ('fence', 'easy', 'oak', '')):
        apply_novelty(k12, *one)
    named = [('pogo9', make_spec(T.POGO, 9)), ('pogo10', make_spec(T.POGO, 10)), ('axe10', T.build_spec('axe10')),
             ('stk_add_repl12', T.build_spec('stk_add_repl12')), ('k12', k12), ('pogo36', make_spec(T.POGO, 36)), ('pogo48', make_spec(T.POGO, 48))]
    residues = []
    for name, spec in named:
        path = os.path.join(tmp, name + '.spec')
        compiled = spec.compile()
        with open(path, 'wb') as f:
            f.write(bytes(compiled))
        specs.append(path)
        residues.append(compiled.n_items % 4)
    assert sorted(set(residues[:5])) == [0, 1, 2, 3]
    return {'ok': os.path.join(BUILD, 'hostcheck'), 'short': os.path.join(BUILD, 'hostcheck_short'), 'specs': specs[:5], 'big': specs[5:7]}


def _run(exe, scenario, specs, *more):
    if scenario == 'refusals':
        specs = list(specs)[:1] + BIG[:2]
    return subprocess.run([exe, scenario] + list(specs) + list(more), capture_output=True, text=True, timeout=TIMEOUT, env=_env())


BIG = []


@pytest.mark.parametrize('scenario', SCENARIOS)
def test_scenario_is_clean(hostcheck, scenario):
    BIG[:] = hostcheck['big']
    specs = hostcheck['specs'] if scenario in ('search', 'tree') else hostcheck['specs'][1:2]
    r = _run(hostcheck['ok'], scenario, specs)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "scenario '%s' passed" % scenario in r.stdout
    reached = {line.split()[1] for line in r.stderr.splitlines() if line.startswith('stub ')}
    missing = [s for s in MUST_REACH.get(scenario, []) if s not in reached]
    assert not missing, 'scenario %s never reached %s' % (scenario, missing)


@pytest.mark.parametrize('scenario', [s for s in SCENARIOS if s not in ('search', 'tree')])
def test_other_specs_are_clean(hostcheck, scenario):
    """every scenario on the odd map (9 x 9) and on a configuration with reset passes and 11 items (`search` and `tree` run every spec above)"""
    BIG[:] = hostcheck['big']
    for spec in (hostcheck['specs'][0], hostcheck['specs'][3], hostcheck['specs'][4]):
        r = _run(hostcheck['ok'], scenario, [spec])
        assert r.returncode == 0, spec + '\n' + r.stdout[-2000:] + r.stderr[-6000:]


def _check_picked(r, allocation):
    lines = [line for line in r.stderr.splitlines() if line.startswith('fake_hip: the picked allocation:')]
    assert len(lines) == 1, lines
    if allocation in PICKED_BYTES:
        assert int(lines[0].split(':')[2].split()[0]) == PICKED_BYTES[allocation], lines[0]


@pytest.mark.parametrize('scenario,allocation', MUST_TRIP)
def test_short_allocation_trips(hostcheck, scenario, allocation):
    r = _run(hostcheck['short'], scenario, hostcheck['specs'][1:2], 'short=' + allocation)
    assert r.returncode != 0, 'the allocation %s, 8 bytes short, went unnoticed: a hole in a stub' % allocation
    assert 'ERROR: AddressSanitizer' in r.stderr, r.stderr[-3000:]
    _check_picked(r, allocation)


@pytest.mark.parametrize('scenario,allocation,rule', ROUNDED_UP)
def test_rounded_up_allocation_holds(hostcheck, scenario, allocation, rule):
    r = _run(hostcheck['short'], scenario, hostcheck['specs'][1:2], 'short=' + allocation)
    assert r.returncode == 0, rule + '\n' + r.stderr[-3000:]
    _check_picked(r, allocation)


@pytest.mark.parametrize('scenario', ['search', 'table', 'snapshot'])
def test_every_allocation_short_aborts(hostcheck, scenario):
    """With EVERY allocation short the first report comes from ngw_create, whatever the scenario: the upload of the spec blob into an allocation of
    exactly sizeof(NgwDevSpec).  So this shows that the all-short build aborts, and nothing about the three scenarios beyond it - what each of their
    slabs does when short is test_short_allocation_trips."""
    r = _run(hostcheck['short'], scenario, hostcheck['specs'][1:2])
    assert r.returncode != 0
    assert 'ERROR: AddressSanitizer' in r.stderr, r.stderr[-3000:]
    report = r.stderr[r.stderr.index('ERROR: AddressSanitizer'):]
    assert ' in ngw_create ' in report[:report.index('is located')], report[:3000]


def test_short_build_is_clean_with_nothing_short(hostcheck):
    r = _run(hostcheck['short'], 'table', hostcheck['specs'][1:2], 'short=none')
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(hostcheck['short'], 'table', hostcheck['specs'][1:2], 'short=no_such_allocation')
    assert r.returncode == 3, 'an allocation name that no scenario arms must not pass silently'


def test_ledger_catches_a_leak(hostcheck):
    r = _run(hostcheck['ok'], 'leak_selfcheck', hostcheck['specs'][1:2])
    assert r.returncode != 0
    assert 'the ledger is not empty' in r.stderr and 'device allocation' in r.stderr and '24 bytes' in r.stderr, r.stderr[-3000:]
