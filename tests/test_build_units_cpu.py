"""CPU: the include lists of `build.UNITS` are what the sources include.  An object in build/obj is reused while the hash of
its unit's source, of the listed `.hip` fragments and of the headers stands: a fragment missing from a list would leave a
stale object behind an edit, a `.hip` outside every unit would never be compiled."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from meshdqn_amd import build  # noqa: E402

INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+\.hip)"', re.M)


def _reached(src):
    """`.hip` files reached from `src` through #include "....hip", transitively (names relative to csrc/), without `src`."""
    seen, todo = set(), [src]
    while todo:
        with open(os.path.join(build.CSRC, todo.pop())) as f:
            for inc in INCLUDE.findall(f.read()):
                inc = os.path.normpath(inc)
                if inc not in seen:
                    seen.add(inc)
                    todo.append(inc)
    return seen


def test_include_lists_match_the_sources():
    for name, (src, _flags, incs) in build.UNITS.items():
        assert len(set(incs)) == len(incs), (name, incs)
        assert _reached(src) == set(incs), (name, sorted(_reached(src)), sorted(incs))


def test_every_hip_file_belongs_to_a_unit():
    owned = set()
    for src, _flags, incs in build.UNITS.values():
        owned |= {src, *incs}
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}
    assert on_disk == owned, (sorted(on_disk - owned), sorted(owned - on_disk))
