"""Source audit of the host side's two bookkeeping rules (csrc/ngw_host.h): the flags that say whether a derived copy still describes the
state in HBM are dropped in ONE place, state_written(), and nothing reaches launch() through fields of the handle.  Parses the sources
like test_solo_stop_audit.py does.  No GPU needed."""
import os
import re

from test_solo_stop_audit import CSRC, _strip, parse

# functions that may take validity away: state_written itself, the public invalidation call, and the switch of the boards mode (every
# bit row is stale when it comes on)
DROPPERS = {'state_written', 'ngw_host_mirror_invalidate', 'boards_mode_changed'}
DROP = re.compile(r'\b(?:solo_mirror_valid|mirror_valid|act_mask_fresh)\s*=\s*false\b|\bbrd_dirty\s*=\s*true\b')
GONE = ('launch_seq', 'launch_action0', 'launch_use_action0', 'launch_act_u8', 'launch_wire', 'act_mask_defer')


def test_only_state_written_drops_the_derived_state_flags():
    funcs = parse()
    assert any(name == 'state_written' for name, _ in funcs)
    bad = sorted((name, fn, m.group(0)) for (name, fn), body in funcs.items() if name not in DROPPERS for m in DROP.finditer(body))
    assert not bad, "derived-state flags dropped outside state_written(): %s" % bad
    # the pattern does see what it is meant to see
    body = [b for (name, _), b in funcs.items() if name == 'state_written'][0]
    assert len(DROP.findall(body)) == 4


def test_nothing_is_passed_to_launch_through_the_handle():
    text = {fn: _strip(open(os.path.join(CSRC, fn)).read()) for fn in sorted(os.listdir(CSRC)) if fn.endswith(('.cpp', '.h'))}
    for word in GONE:
        hits = [fn for fn, t in text.items() if re.search(r'\b%s\b' % word, t)]
        assert not hits, "%s is back in %s" % (word, hits)
    rollout = [b for (name, _), b in parse().items() if name == 'rollout_chunks'][0]
    assert 'launch(' in rollout and not re.search(r'\bproto\.\w+\s*=[^=]', rollout), "rollout_chunks edits the handle's launch prototype"


def test_no_bare_literal_in_a_feat_argument():
    for (name, fn), body in parse().items():
        for call in re.findall(r'\bngw_launch\s*\(([^;]*);', body):
            feat = call.split(',')[3]
            assert not re.search(r'(?<![\w.])[1-9]\d*\b', feat), "%s (%s): feat argument %r" % (name, fn, feat.strip())
