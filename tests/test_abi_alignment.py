"""The validators of the C ABI against tests/abi_alignment.py, on the CPU:
made-up pointer values that are never dereferenced (every call returns from
its argument checks, or is an empty batch).

* accepted at the minimum: every pointer of a call at a 16-byte-aligned value
  plus exactly its minimum (so an argument whose minimum is 4 is NOT 8- or
  16-byte aligned) — G2K_OK, or for the entry points that have no HIP-free
  success the size check that follows the alignment checks;
* rejected below it: the same call with ONE state-"a" pointer at half its
  minimum is G2K_EINVAL and the message names the argument;
* the table covers the headers (include/g2k_hip.h, and the two that declare
  what is bound by symbol: include/g2k_mix.h, include/g2k_scores.h): every
  declared entry point and every pointer parameter of it, with the check or
  branch each row quotes present in the source it names, and the header that
  declares an entry point stating every validated requirement in that entry
  point's "Alignment (bytes) of ..." sentence.

Every symbol is reached through the binding that sets its argument types:
_lib.load() for g2k_hip.h, mixture.load() for g2k_mix.h, scores.load() for
g2k_scores.h.
"""
import ctypes
import os
import re

import pytest

from multimodaltraj_2_amd import _lib, mixture, scores
from tests import abi_alignment as al
from tests.test_abi import HEADER, ROOT, declared_functions

CSRC = os.path.join(ROOT, "multimodaltraj_2_amd", "csrc")
EINVAL = -1
# header -> the binding of its symbols
BINDINGS = {HEADER: _lib.load,
            os.path.join(ROOT, "include", "g2k_mix.h"): mixture.load,
            os.path.join(ROOT, "include", "g2k_scores.h"): scores.load}
HEADERS = tuple(BINDINGS)


def uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)


def declared_in():
    """{function: the header that declares it}; no function is declared twice."""
    out = {}
    for h in HEADERS:
        for fn in set(re.findall(r"\b(g2k_[a-z0-9_]+)\s*\(", uncommented(h))):
            assert fn not in out, (fn, h, out[fn])
            out[fn] = h
    return out


DECLARED_IN = declared_in()


def bound(entry):
    """The library handle, through the binding of the header that declares `entry`."""
    return BINDINGS[DECLARED_IN[entry.name]]()


def resolve(entry, cond):
    """{arg name: (min, state)} and the dims of `entry` under `cond` (a label
    of one of its args' conditions, or None)."""
    dims, req = dict(entry.dims), {}
    for a in entry.args:
        if a.cond and a.cond[0] == cond:
            dims.update(a.cond[1])
            req[a.name] = (a.cond[2], a.cond[3])
        else:
            req[a.name] = (a.min, a.state)
    return dims, req


def call(lib, entry, cond, moved=None):
    """Call `entry` with every pointer at 65536 k + its minimum (a different k
    per argument; no two ranges an entry point checks for overlap meet: the
    mixture block is 19456 bytes), `moved` = (name, offset) at 65536 k + offset
    instead."""
    dims, req = resolve(entry, cond)
    keep, k = [], [0]

    def value(a):
        k[0] += 1
        off = moved[1] if moved and moved[0] == a.name else req[a.name][0]
        return 65536 * k[0] + off

    argv = []
    for p in entry.params:
        if p == "dims":
            keep.append(_lib.G2KDims(**dims))
            argv.append(ctypes.byref(keep[-1]))
        elif p == "weights":
            keep.append(_lib.G2KWeights(**{a.name: value(a) for a in entry.weights}))
            argv.append(ctypes.byref(keep[-1]))
        elif isinstance(p, al.Arg):
            argv.append(value(p))
        else:
            argv.append(p.value)
    rc = getattr(lib, entry.name)(*argv)
    return rc, (lib.g2k_last_error() or b"")


CASES = [(e, c) for e in al.ENTRIES for c in (None,) + tuple(dict.fromkeys(e.conditions()))]
CASE_IDS = [e.name + ("" if c is None else "-" + c) for e, c in CASES]


@pytest.mark.parametrize("entry,cond", CASES, ids=CASE_IDS)
def test_accepted_at_the_minimum(entry, cond):
    lib = bound(entry)
    rc, msg = call(lib, entry, cond)
    if entry.accept == "ok":
        assert rc == 0, (rc, msg)
    else:       # past every alignment check, to the size check behind them
        assert rc == EINVAL and b"bytes needed" in msg and b"aligned" not in msg, (rc, msg)


REJECTIONS = [(e, c, a.name) for e, c in CASES for a in e.args if resolve(e, c)[1][a.name][1] == "a"]


@pytest.mark.parametrize("entry,cond,name", REJECTIONS,
                         ids=[e.name + ("" if c is None else "-" + c) + "-" + n for e, c, n in REJECTIONS])
def test_rejected_below_the_minimum(entry, cond, name):
    lib = bound(entry)
    need = resolve(entry, cond)[1][name][0]
    arg = next(a for a in entry.args if a.name == name)
    rc, msg = call(lib, entry, cond, moved=(name, need // 2))
    assert rc == EINVAL, (rc, msg)
    assert (arg.word or name).encode() in msg and b"%d-byte aligned" % need in msg, msg
    # ... and the twin with that pointer back at its minimum is the accepted call
    rc, msg = call(lib, entry, cond, moved=(name, need))
    assert (rc == 0) if entry.accept == "ok" else (b"bytes needed" in msg), (rc, msg)


def test_no_pointer_sits_below_its_natural_alignment_or_above_16():
    for e in al.ENTRIES:
        for a in e.args:
            for need, state in ((a.min, a.state),) + (((a.cond[2], a.cond[3]),) if a.cond else ()):
                assert need in (1, 2, 4, 8, 16) and need >= al.ELEM_BYTES[a.elem], (e.name, a.name)
                assert state in ("a", "b", "c"), (e.name, a.name)
                # natural means natural; more than that is validated or branched on
                assert state != "c" or need == al.ELEM_BYTES[a.elem], (e.name, a.name)


def test_every_quoted_check_is_in_the_source():
    src = {}
    for e in al.ENTRIES:
        for a in e.args:
            quoted = [(a.state, a.where)] + ([(a.cond[3], a.cond[4])] if a.cond else [])
            quoted += [("b", a.branch)] if a.branch else []
            for state, where in quoted:
                if state == "c":
                    assert not where, (e.name, a.name)
                    continue
                assert where, (e.name, a.name, "a validated / handled row quotes its check")
                f, text = where
                if f not in src:
                    src[f] = open(os.path.join(CSRC, f)).read()
                assert text in src[f], (e.name, a.name, f, text)


def prototypes():
    """{function: [(type, name), ...]} of the three headers' declarations."""
    out = {}
    for h in HEADERS:
        for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", uncommented(h)):
            params = []
            for p in m.group(2).split(","):
                p = " ".join(p.split())
                if p and p != "void":
                    t, n = p.rsplit(" ", 1)
                    params.append((t, n))
            assert m.group(1) not in out and DECLARED_IN[m.group(1)] == h, m.group(1)
            out[m.group(1)] = params
    return out


def test_table_covers_every_pointer_of_every_entry_point():
    protos = prototypes()
    assert sorted(list(al.BY_NAME) + list(al.NO_DEVICE_POINTERS)) == sorted(DECLARED_IN)
    assert sorted(protos) == sorted(DECLARED_IN)           # every declaration parsed as a prototype
    assert sorted(fn for fn, h in DECLARED_IN.items() if h == HEADER) == declared_functions()
    for h, n in ((HEADERS[1], 9), (HEADERS[2], 5)):        # what g2k_mix.h and g2k_scores.h declare
        assert sum(v == h for v in DECLARED_IN.values()) == n, h
    for e in al.ENTRIES:
        want = [n for t, n in protos[e.name] if "*" in t and n not in ("d", "w", "stream")]
        got = [p.name for p in e.params if isinstance(p, al.Arg)]
        assert got == want, (e.name, got, want)
        # and the parameters as a whole, in order (d / w are the structs)
        names = [{"dims": "d", "weights": "w"}[p] if isinstance(p, str) else p.name for p in e.params]
        assert names == [n for _, n in protos[e.name]], (e.name, names)
    members = re.search(r"typedef struct g2k_weights \{(.*?)\} g2k_weights;", open(HEADER).read(), re.S)
    fields = re.findall(r"const float\* (\w+);", members.group(1))
    for e in al.ENTRIES:
        assert {a.name for a in e.weights} <= set(fields), e.name


def alignment_sentences():
    """{entry point: text} of the headers' "Alignment (bytes) of A[, B and C]:
    ... ." sentences (inside comments); an entry point's sentence stands in the
    header that declares it."""
    out = {}
    for h in HEADERS:
        for block in re.findall(r"/\*.*?\*/", open(h).read(), flags=re.S):
            flat = " ".join(line.strip().lstrip("*").strip() for line in block.splitlines())
            for m in re.finditer(r"Alignment \(bytes\) of ([^:]*):(.*?)\.(?= |$)", flat):
                for fn in re.findall(r"g2k_[a-z0-9_]+", m.group(1)):
                    assert fn not in out, fn
                    assert DECLARED_IN.get(fn) == h, (fn, "sentence in", h, "declared in", DECLARED_IN.get(fn))
                    out[fn] = m.group(2)
    return out


def test_header_states_every_validated_requirement():
    sentences = alignment_sentences()
    text = open(HEADER).read()
    assert "natural alignment of its element type" in " ".join(text.split())
    for e in al.ENTRIES:
        rows = [(a.name, a.min, a.state, "") for a in e.args]
        rows += [(a.name, a.cond[2], a.cond[3], a.cond[0]) for a in e.args if a.cond]
        for name, need, state, cond in rows:
            if state != "a":
                continue
            assert e.name in sentences, (e.name, "no Alignment (bytes) sentence")
            assert re.search(r"\b%s %d\b" % (re.escape(name), need), sentences[e.name]), \
                (e.name, name, need, sentences[e.name])
    # and nothing the table does not hold: every "name N" of a sentence is a row
    for fn, s in sentences.items():
        e = al.BY_NAME[fn]
        known = {(a.name, a.min) for a in e.args} | {(a.name, a.cond[2]) for a in e.args if a.cond}
        for name, need in re.findall(r"\b([A-Za-z_][A-Za-z_0-9]*) (\d+)\b", s):
            assert (name, int(need)) in known, (fn, name, need)
