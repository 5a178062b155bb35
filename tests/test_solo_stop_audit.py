"""Source audit of the one-env resident step loop's rule (csrc/ngw_host.h, solo_stop): while the loop runs, the handle's state in HBM
is only correct once the loop has committed the last posted action, and its stream is busy until the loop ends.  So every C-ABI entry
point that uses the handle's stream or its device state must end the loop first - by calling solo_stop itself, or a helper whose own
body does (launch, rollout_chunks, ...).  The helpers are resolved by parsing the sources, not by a list.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_novel_gridworlds_amd', 'csrc')

# a use of the handle's stream or its device memory
USES = re.compile(r'\bh->stream2?\b|\bhipStreamSynchronize\b|\bhipMemcpy\w*|\bhipMemset\w*|\b\w+_launch\s*\(')
STOP = re.compile(r'\bsolo_stop\s*\(')
# calls that are neither a use nor a stop: the loop's own protocol (a step through it, its records of the masks), and ngw_destroy (the
# handle is gone afterwards: calling it on an error path ends nothing that the caller goes on using)
NEUTRAL = {'solo_stop', 'solo_step', 'solo_mask', 'ngw_destroy'}

# Entry points that use the stream or the state without ending the loop, each for a stated reason.
ALLOW = {
    'ngw_create': 'creates the handle: no resident loop can be running on it yet',
}

# Entry points that touch neither the stream nor the device state (pure getters, host memory, error text): nothing to stop.
NO_STREAM = {
    'ngw_abi_version', 'ngw_spec_size', 'ngw_last_error', 'ngw_device_count', 'ngw_host_alloc', 'ngw_host_free',
    'ngw_obs_device_ptrs', 'ngw_out_device_ptrs', 'ngw_terminal_device_ptrs', 'ngw_lidar_device_ptr', 'ngw_agent_view_device_ptr',
    'ngw_lidar_row_layout', 'ngw_host_step_layout', 'ngw_host_step_layout_packed', 'ngw_pack_layout', 'ngw_host_mirror_invalidate',
    'ngw_get_reset_prefetch', 'ngw_get_reset_prefetch_depth', 'ngw_step_kernel_info', 'ngw_debug_refill_cadence', 'ngw_debug_solo_starts',
}


def _strip(text):
    """Comments and the contents of string / character literals out (newlines kept), so that braces and words in them do not count."""
    def repl(m):
        s = m.group(0)
        if s[0] in '"\'':
            return s[0] + s[0]
        return '\n' * s.count('\n') or ' '
    return re.sub(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', repl, text, flags=re.S)


DEF = re.compile(r'^(?!(?:namespace|extern|using|struct|class|typedef|static_assert|template)\b)[A-Za-z_][^;{}()\n]*?\b([A-Za-z_]\w*)\s*\([^;{}]*\)\s*(?:const\s*)?\{',
                 re.M)
MACRO = re.compile(r'^#define\s+(\w+)\(([^)]*)\)((?:[^\n]*\\\n)*[^\n]*)', re.M)


def parse(csrc=CSRC):
    """{(name, file): body} of every function defined at file scope in ngw_abi_*.cpp and ngw_host.h, and of the function-like macros of
    ngw_host.h (HIP_TRY, D2H, H2D).  (A helper in an anonymous namespace may have a namesake in another file: the file is part of the key.)"""
    funcs = {}
    files = sorted(f for f in os.listdir(csrc) if f.startswith('ngw_abi_') and f.endswith('.cpp')) + ['ngw_host.h']
    for fn in files:
        text = _strip(open(os.path.join(csrc, fn)).read())
        for m in MACRO.finditer(text):
            funcs[(m.group(1), fn)] = m.group(3)
        for m in DEF.finditer(text):
            depth, i = 1, m.end()
            while depth:
                c = text[i]
                depth += (c == '{') - (c == '}')
                i += 1
            assert (m.group(1), fn) not in funcs, "%s defined twice in %s" % (m.group(1), fn)
            funcs[(m.group(1), fn)] = text[m.end():i - 1]
    return funcs


def classify(funcs):
    """{name: (uses, stops, first)} of every function with ONE definition: uses - its body, or a function or macro it calls, uses the
    stream or device memory; stops - its body, or a function it calls, calls solo_stop; first - the first stopping call in its body comes
    before its first use.  A call resolves to the callee in the caller's own file, else to every definition of that name."""
    by_name = {}
    for (f, fn) in funcs:
        by_name.setdefault(f, []).append((f, fn))

    def resolve(c, fn):
        return [(c, fn)] if (c, fn) in funcs else by_name[c]
    calls = {k: {c for c in re.findall(r'\b([A-Za-z_]\w*)\s*\(', body) if c in by_name and c != k[0] and c not in NEUTRAL}
             for k, body in funcs.items()}
    uses = {k: bool(USES.search(body)) for k, body in funcs.items()}
    stops = {k: bool(STOP.search(body)) for k, body in funcs.items()}
    changed = True
    while changed:                                   # (transitive closure over the call graph)
        changed = False
        for k in funcs:
            u = uses[k] or any(uses[d] for c in calls[k] for d in resolve(c, k[1]))
            s = stops[k] or any(all(stops[d] for d in resolve(c, k[1])) for c in calls[k])
            if (u, s) != (uses[k], stops[k]):
                uses[k], stops[k], changed = u, s, True
    out = {}
    for k, body in funcs.items():
        stop_at = [m.start() for m in STOP.finditer(body)]
        use_at = [m.start() for m in USES.finditer(body)]
        for c in calls[k]:
            at = [m.start() for m in re.finditer(r'\b%s\s*\(' % c, body)]
            ds = resolve(c, k[1])
            if all(stops[d] for d in ds):
                stop_at += at
            elif any(uses[d] for d in ds):
                use_at += at
        first = not use_at or (bool(stop_at) and min(stop_at) < min(use_at))
        if len(by_name[k[0]]) == 1:
            out[k[0]] = (uses[k], stops[k], first)
    return out


def header_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ngw.h')).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(ngw_[a-z_0-9]+)\s*\(', text)))


def violation(cls, f):
    """Why entry point f breaks the rule, or None."""
    uses, stops, first = cls[f]
    if uses and not stops:
        return 'uses the stream / device state without ending the one-env loop (solo_stop)'
    if uses and not first:
        return 'uses the stream / device state before it ends the one-env loop'
    return None


def audit(csrc=CSRC):
    """Entry points that break the rule and are not on the allow-list: [(name, why)]."""
    cls = classify(parse(csrc))
    return [(f, violation(cls, f)) for f in sorted(cls) if f.startswith('ngw_') and f not in ALLOW and violation(cls, f)]


def test_parser_finds_the_entry_points_and_resolves_helpers():
    funcs = parse()
    cls = classify(funcs)
    assert len([f for f in cls if f.startswith('ngw_')]) >= 70
    for helper in ('launch', 'rollout_chunks', 'capture_graph'):     # helpers that end the loop on their callers' behalf
        assert cls[helper][:2] == (True, True), helper
    for helper in ('dev_alloc', 'rebuild_boards', 'upload_reset_u', 'D2H', 'H2D'):   # ... and some that only use the stream
        assert cls[helper][:2] == (True, False), helper
    assert cls['HIP_TRY'][0] is False and cls['solo_stop'][0] is True
    assert funcs[('ngw_abi_version', 'ngw_abi_create.cpp')].strip() == 'return NGW_ABI_VERSION;'      # (a one-line body)


def test_every_entry_point_ends_the_one_env_loop_before_it_uses_the_stream():
    bad = audit()
    assert not bad, "entry points that break ngw_host.h's solo_stop rule:\n" + '\n'.join('  %s: %s' % b for b in bad)


def test_every_declared_entry_point_is_classified():
    """Every ngw_* function include/ngw.h declares is defined once in ngw_abi_*.cpp (so the audit above sees it), and each entry point
    either ends the loop, or is on the allow-list with a reason, or is one of the named functions that touch neither the stream nor the state."""
    cls = classify(parse())
    missing = [s for s in header_symbols() if s not in cls]
    assert not missing, "declared in include/ngw.h but not found (once) in csrc/ngw_abi_*.cpp: %s" % missing
    entry = {f for f in cls if f.startswith('ngw_')}
    assert set(ALLOW) <= entry and NO_STREAM <= entry, (set(ALLOW) - entry, NO_STREAM - entry)
    no_stream = {f for f in entry if not cls[f][0]}
    assert no_stream == NO_STREAM, ("touch neither the stream nor the state - name them in NO_STREAM: %s" % sorted(no_stream - NO_STREAM),
                                    "listed in NO_STREAM but use the stream or the state: %s" % sorted(NO_STREAM - no_stream))
    for f, why in ALLOW.items():
        assert why and violation(cls, f), "%s: stale allow-list entry (it follows the rule)" % f
