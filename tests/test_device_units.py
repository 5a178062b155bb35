"""Source audit of the device code's layout (csrc/ngw_unit_*.hip, csrc/ngw_common.inc): the library is one compilation unit per
ngw_unit_<name>.hip, each starting from the common prelude, and every launcher the host side calls (the `hipError_t ngw_*(` declarations of
csrc/ngw_device.h) is defined in exactly one place, so the units link without a clash and without a missing symbol.  Nothing is compiled.
No GPU needed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gym_novel_gridworlds_amd', 'csrc')


def _strip(text):
    """Comments out (newlines kept), so that a launcher named in prose does not count."""
    return re.sub(r'//[^\n]*|/\*.*?\*/', lambda m: '\n' * m.group(0).count('\n') or ' ', text, flags=re.S)


def _read(path):
    with open(path) as f:
        return _strip(f.read())


def declared():
    """The launchers of ngw_device.h: every `hipError_t ngw_*(` that ends in `;`."""
    return re.findall(r'\bhipError_t\s+(ngw_\w+)\s*\([^;{}]*\)\s*;', _read(os.path.join(CSRC, 'ngw_device.h')))


def definitions():
    """{name: [files]} of every `hipError_t ngw_*(...) {` in csrc/*.hip and csrc/*.inc."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.inc'))):
        for name in re.findall(r'\bhipError_t\s+(ngw_\w+)\s*\([^;{}]*\)\s*\{', _read(path)):
            found.setdefault(name, []).append(os.path.basename(path))
    return found


def units():
    return sorted(glob.glob(os.path.join(CSRC, 'ngw_unit_*.hip')))


def test_every_declared_launcher_is_defined_once():
    names = declared()
    assert len(names) >= 28 and len(set(names)) == len(names), names     # (the parser found them - 28 when this was written - each once)
    defs = definitions()
    wrong = {n: defs.get(n, []) for n in names if len(defs.get(n, [])) != 1}
    assert not wrong, "declared in ngw_device.h but not defined exactly once in csrc/*.hip, csrc/*.inc: %s" % wrong


def test_every_unit_includes_the_common_prelude():
    assert units(), "no csrc/ngw_unit_*.hip"
    missing = [os.path.basename(p) for p in units() if not re.search(r'^#include "ngw_common\.inc"', _read(p), re.M)]
    assert not missing, 'units without #include "ngw_common.inc": %s' % missing
