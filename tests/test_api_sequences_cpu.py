"""The call sequences of tests/test_gpu_api_sequences.py, without a GPU: `sequence(seed)` is a pure function, and for
every committed seed it reaches every op of the vocabulary at least twice and every producer of the matrix at least five
times; every op of the vocabulary has its branch in `Rig._call`, and every op added there calls the binding's method, or
the package's function on an engine, of that name; no public method or engine-level function is left unnamed.  And what
no sequence of two engines of the same code can see: the target's transitions themselves (csrc/ndt_target_state.*),
walked under sanitizers as a stand-alone program, and who may call them."""
import collections
import inspect
import os
import re
import subprocess

import pytest

import test_gpu_api_sequences as api
from test_gpu_api_sequences import (CONSUMERS, GRID_CONSUMERS, KEEP_GRID_CONSUMERS, LENGTH, MODULE_OPS, NEW_OPS, OLD_OPS, OPS,
                                    PRODUCER_OPS, SEEDS, SERVED_TWICE, TABLE_PRODUCERS, Rig, sequence)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-sam_amd", "csrc")


@pytest.mark.parametrize("seed", SEEDS)
def test_every_op_twice_and_every_producer_five_times(seed):
    seq = sequence(seed)
    assert seq == sequence(seed) and len(seq) == LENGTH            # pure: the same list again
    assert all(op in OPS and 0 <= k < 24 for op, k in seq)
    n = collections.Counter(op for op, _ in seq)
    rare = {op: n[op] for op in OPS if n[op] < 2}
    assert not rare, rare
    few = {op: n[op] for op in PRODUCER_OPS if n[op] < 5}
    assert not few, few


def test_seeds_give_different_sequences():
    assert len({tuple(sequence(s)) for s in SEEDS}) == len(SEEDS) == 3


def test_vocabulary_is_handled_and_complete(pkg):
    """every op has a branch in Rig._call, no op is listed twice, every consumer of the matrix is an op, and every new op
    that is a method of the binding is really called by name"""
    assert len(set(OPS)) == len(OPS) and len(OLD_OPS) == 24
    src = inspect.getsource(Rig._call)
    for op in OPS:
        assert '"%s"' % op in src, op
    methods = {m for m, _ in inspect.getmembers(pkg.NormalDistributionsTransform, inspect.isfunction)}
    for op in NEW_OPS:
        assert op in methods and "e.%s(" % op in src, op
    functions = engine_functions(pkg)
    for op in MODULE_OPS:                                          # a function of the package on an engine, called as one
        assert op in functions and "pkg.%s(e" % op in src, op
    assert {op for op, _ in CONSUMERS} == set(NEW_OPS) | set(MODULE_OPS)
    assert {op for op, _ in KEEP_GRID_CONSUMERS} <= set(OPS) and {op for op, _ in GRID_CONSUMERS} <= set(OPS)
    assert len(set(KEEP_GRID_CONSUMERS)) == len(KEEP_GRID_CONSUMERS) and not set(KEEP_GRID_CONSUMERS) & set(GRID_CONSUMERS)
    # the deferred-failure test holds every engine-level function but the two that replace the target
    held = {op for op, _ in KEEP_GRID_CONSUMERS} | {op for op, _ in GRID_CONSUMERS}
    assert set(MODULE_OPS) - held == {"setInputTargetFromMapLevel", "alignMapLevels"}
    assert {"setInputTargetFromMapLevel", "alignMapLevels"} <= {op for op, _, _ in TABLE_PRODUCERS}
    assert set(SERVED_TWICE) <= set(MODULE_OPS)
    # MODULE_OPS is every such function but the reads named as left out and second names of the same function
    names = {f.__name__ for f in functions.values()}               # (a second name has the `def`'s __name__)
    assert set(MODULE_OPS) == names - LEFT_OUT_READS, (set(MODULE_OPS) ^ (names - LEFT_OUT_READS))


LEFT_OUT_READS = {"sourceDistributionsInfo", "sourceTimesInfo", "getScanContextParams", "scanContextBankCount"}


def engine_functions(pkg):
    """name -> function: the package's public module-level functions whose first parameter is named `ndt`"""
    out = {}
    for name, f in inspect.getmembers(pkg, inspect.isfunction):
        if name.startswith("_") or f.__module__ != pkg.__name__:
            continue
        params = list(inspect.signature(f).parameters)
        if params and params[0] == "ndt":
            out[name] = f
    return out


def test_the_time_edits_are_drawn_in_the_committed_seeds():
    """setSourceTimes with one NaN (k % 8 == 5), with the wrong length (6) and empty (7) each occur in the committed seeds"""
    ks = {k % 8 for s in SEEDS for op, k in sequence(s) if op == "setSourceTimes"}
    assert {5, 6, 7} <= ks, ks


def test_every_public_method_is_called_or_named_with_a_reason(pkg):
    """every public method of NormalDistributionsTransform, and every public function of the package on an engine, is
    either called on an engine by the rig (`e.<name>(`, `pkg.<name>(e`) or named in the module's list of what is left out"""
    rig_src, doc = inspect.getsource(Rig), api.__doc__
    left_out = doc[doc.index("NOT in the vocabulary"):]
    missing = []
    for name, _ in inspect.getmembers(pkg.NormalDistributionsTransform, inspect.isfunction):
        if name.startswith("_"):
            continue
        called = "e.%s(" % name in rig_src
        named = re.search(r"(?<![A-Za-z_])%s(?![A-Za-z_])" % re.escape(name), left_out) is not None
        if not (called or named):
            missing.append(name)
    assert not missing, missing
    # ... and so is every public function of the package that takes the engine as its first argument `ndt` (called as
    # `pkg.<name>(e`); another name bound to the same function counts with it
    functions = engine_functions(pkg)
    assert functions["computeDerivativesD2D"] is functions["evalDerivativesD2D"] and "alignMapLevels" in functions
    for name, f in functions.items():
        same = [n for n, g in functions.items() if g is f]
        called = any("pkg.%s(e" % n in rig_src for n in same)
        named = any(re.search(r"(?<![A-Za-z_])%s(?![A-Za-z_])" % re.escape(n), left_out) is not None for n in same)
        if not (called or named):
            missing.append(name)
    assert not missing, missing


# --------------------------------------------------------------------------- the target's state and its transitions
def test_target_state_transitions_under_asan_ubsan(tmp_path):
    """tests/cpp/sanitize_target_state.cpp (its own main) + csrc/ndt_target_state.cpp under ASan + UBSan as a child process:
    every transition from every reachable state, 10^5 random ones, the reduced fuzz sequence replayed.  Never through
    Python's loader."""
    exe = str(tmp_path / "sanitize_target_state")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                        "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "sanitize_target_state.cpp"),
                        os.path.join(CSRC, "ndt_target_state.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("PASS"), r.stdout[-2000:]


def test_the_target_changes_through_three_wrappers_only():
    """The state's fields are private to ndt_target_state.*; its transitions are called by target_retire, target_publish
    and target_drop (ndt_handoff.hip) and by nobody else; the loose fields they replaced are gone, and the engine's own
    cloud is freed by target_retire and ndt_destroy alone.  (claim_cloud is the producers' own call: it stands in front of
    their first write to tx/ty/tz.)"""
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp"))}
    state = ("ndt_target_state.h", "ndt_target_state.cpp")
    fields = re.findall(r"\b(\w+_)\b(?= = |,|;)", sources[state[0]][sources[state[0]].index(" private:"):])
    assert sorted(set(fields)) == ["cloud_n_", "gen_", "kind_", "n_points_", "n_slots_", "n_valid_", "prev_n_valid_", "reuse_"], fields
    for f in state:                                              # host only: no HIP type, no HIP header
        assert not re.search(r"\bhip[A-Z_]\w*|#include\s*[<\"]hip|ndt_engine\.h\"", sources[f]), f

    def enclosing(text, pos):
        heads = re.findall(r"^(?:[\w:]+ )+\*?(\w+)\([^;{]*?\) \{", text[:pos], flags=re.M | re.S)
        return heads[-1] if heads else None

    for f, text in sources.items():
        if f in state:
            continue
        for name in fields:                                      # no file but the state's own names a field
            assert not re.search(r"\b%s\b" % name, text), (f, name)
        for gone in (r"have_grid\s*=[^=]", r"multi_active", r"\bn_tgt\b", r"\btgt_gen\b", r"grid_clean_cap", r"grid_dirty_slots",
                     r"->prev_n_valid\b", r"->n_valid\b", r"->n_slots\b"):
            assert not re.search(gone, text), (f, gone)
    calls = {"retire": [], "publish_single": [], "publish_union": [], "drop": [], "claim_cloud": []}
    releases = []
    for f, text in sources.items():
        if f in state:
            continue
        for t in calls:
            calls[t] += [(f, enclosing(text, m.start())) for m in re.finditer(r"\btgt\.%s\(" % t, text)]
        releases += [(f, enclosing(text, m.start())) for m in re.finditer(r"\btx\.release\(", text)]
        assert not re.search(r"(?<!tgt)\.(retire|publish_single|publish_union)\(", text), f   # (under no other name either)
    assert calls["retire"] == [("ndt_handoff.hip", "target_retire")]
    assert calls["publish_single"] == calls["publish_union"] == [("ndt_handoff.hip", "target_publish")]
    assert calls["drop"] == [("ndt_handoff.hip", "target_drop")]
    assert sorted(releases) == [("ndt_handle.hip", "ndt_destroy"), ("ndt_handoff.hip", "target_retire")]
    # the producers that fill the engine's own arrays claim them first
    assert sorted(calls["claim_cloud"]) == [("ndt_handoff.hip", "build_grid_handoff"), ("ndt_handoff.hip", "ndt_set_target"),
                                            ("ndt_handoff.hip", "ndt_set_target_soa"), ("ndt_keyframes.hip", "ndt_set_target_from_keyframes"),
                                            ("ndt_map.hip", "ndt_set_target_from_map")]
    for f, fn in calls["claim_cloud"]:
        body = sources[f][sources[f].index(" %s(" % fn):]
        assert body.index("claim_cloud()") < min(body.index(w) for w in ("tx.ensure(", "h->tx,") if w in body), (f, fn)
    # and the wrappers have the callers the design names
    wrappers = {w: sorted({(f, enclosing(text, m.start())) for f, text in sources.items() for m in re.finditer(r"\b%s\(h\b" % w, text)})
                for w in ("target_retire", "target_publish", "target_drop")}
    assert wrappers["target_retire"] == [("ndt_handoff.hip", "build_begin"), ("ndt_keyframes.hip", "ndt_multigrid_create_kdtree"),
                                         ("ndt_map.hip", "target_from_moments")], wrappers
    assert wrappers["target_publish"] == [("ndt_handoff.hip", "build_complete"), ("ndt_keyframes.hip", "ndt_multigrid_create_kdtree"),
                                          ("ndt_map.hip", "target_from_moments")], wrappers
    assert wrappers["target_drop"] == [("ndt_handle.hip", "ndt_debug_sort_pairs"), ("ndt_handle.hip", "ndt_set_params"),
                                       ("ndt_keyframes.hip", "ndt_multigrid_add_target"),
                                       ("ndt_keyframes.hip", "ndt_multigrid_remove_target")], wrappers
