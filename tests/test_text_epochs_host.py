"""The book of the text route's epochs, tickets and info blocks (bgreat_amd/csrc/text_epochs.h), driven without a device: tools/text_epochs_main.cpp
plays it, built on its own under AddressSanitizer + UBSan.  A chain word has 22 bits for its epoch; an epoch outside them is never matched and the
kernels behind the first tile would wait for ever -- so no sequence of calls may be handed one, wherever the hook starts the count."""
import itertools
import os
import subprocess

import pytest

from util import ROOT

MAX = 0x3FFFFF   # BGR_TEXT_EPOCH_MAX
PER_CALL = 3     # kTextEpochsPerCall: parse, format, format again behind a settled launch
HOOKS = [0, MAX - 4, MAX - 3, MAX - 2, MAX - 1, MAX]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """(built with -DNDEBUG: the refusal is an error return, as in a release build; built without: it is an assert)"""
    d = tmp_path_factory.mktemp("text_epochs")
    out = []
    for name, extra in (("text_epochs", ["-DNDEBUG"]), ("text_epochs_assert", [])):
        path = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + extra +
                              [os.path.join(ROOT, "tools", "text_epochs_main.cpp"), "-o", path])
        out.append(path)
    return out


@pytest.fixture(scope="module")
def exe(exes):
    return exes[0]


def play(exe, hook, *calls):
    """-> per call {zero, block, next, tickets, epochs (None where refused), end_block, end_next}"""
    p = subprocess.run([exe, str(hook)] + [str(c) for c in calls], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "ERROR: " not in p.stderr and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[0] == "max %d per_call %d" % (MAX, PER_CALL)
    out = []
    for ln in lines[1:]:
        w = ln.split()
        kv = dict(x.split("=") for x in w[1:] if "=" in x)
        if w[0] == "call":
            out.append(dict(zero=kv["zero"] == "1", block=int(kv["block"]), next=int(kv["next"]), tickets=[int(x) for x in kv["tickets"].split(",")], epochs=[]))
        elif w[0] == "epoch":
            out[-1]["epochs"].append(None if w[1] == "error" else int(w[1]))
        else:
            assert w[0] == "end"
            out[-1].update(end_block=int(kv["block"]), end_next=int(kv["next"]))
    assert len(out) == len(calls)
    return out


@pytest.mark.parametrize("hook", HOOKS)
def test_no_sequence_of_calls_leaves_the_22_bits(exe, hook):
    for seq in itertools.product((2, 3), repeat=4):
        last = hook   # the epoch in use in front of the call: the hook on fresh state, then the last one handed out
        for i, c in enumerate(play(exe, hook, *seq)):
            wrap = MAX - last < PER_CALL   # fewer than three epochs remain
            assert c["zero"] == (i == 0 or wrap), (hook, seq, i)   # a clear exactly then (and on the fresh buffer of the first call), never otherwise
            first = 1 if wrap else last + 1
            assert c["epochs"] == list(range(first, first + seq[i])), (hook, seq, i)   # strictly increasing between two clears, the first one behind a clear is 1
            assert all(1 <= e <= MAX for e in c["epochs"])
            if wrap or i == 0:
                assert c["tickets"] == [0, 0]
            last = c["epochs"][-1]


def test_three_epochs_fit_exactly_behind_the_hook(exe):
    (c,) = play(exe, MAX - 3, 3)
    assert c["epochs"] == [MAX - 2, MAX - 1, MAX] and c["tickets"] == [0, 0]
    a, b = play(exe, MAX - 3, 3, 2)   # the call behind it starts over
    assert b["zero"] and b["epochs"] == [1, 2] and b["tickets"] == [0, 0]
    for hook in (MAX - 2, MAX - 1, MAX):   # the top values of the hook's range: cleared before the first launch
        (c,) = play(exe, hook, 3)
        assert c["zero"] and c["epochs"] == [1, 2, 3]


def test_a_chain_state_that_could_not_be_zeroed_is_asked_for_again(exe):
    a, b, c = play(exe, 0, "2z", 2, 2)   # the first call's clear fails: no launch; the call behind it must clear before its first launch
    assert a["zero"] and a["epochs"] == []
    assert b["zero"] and b["epochs"] == [1, 2] and b["tickets"] == [0, 0] and b["block"] == a["block"]
    assert not c["zero"] and c["epochs"] == [3, 4]


def test_tickets_count_what_the_launches_took(exe):
    a, b, c = play(exe, 0, 3, 2, "r2")
    assert a["tickets"] == [0, 0] and b["tickets"] == [3, 4] and not b["zero"]   # (the player: 3 per parse launch, 2 per format launch)
    assert c["zero"] and c["tickets"] == [0, 0] and c["epochs"] == [1, 2]          # a reallocated buffer: no ticket taken, the hook's epoch again


@pytest.mark.parametrize("hook", [0, MAX - 3])
def test_a_fourth_launch_in_a_call_is_refused(exes, hook):
    (c,) = play(exes[0], hook, 4)
    assert c["epochs"][:3] == [hook + 1, hook + 2, hook + 3] and c["epochs"][3] is None   # the error, not a number
    (c,) = play(exes[0], hook, 5)
    assert c["epochs"][3:] == [None, None]
    p = subprocess.run([exes[1], str(hook), "4"], capture_output=True, text=True, timeout=60)   # with asserts: the program stops there
    assert p.returncode != 0 and "epochs reserved" in p.stderr


def test_the_flip_is_committed_behind_the_parse_launch_only(exe):
    a, b, c, d = play(exe, 0, 2, "2x", 2, 3)
    for x in (a, b, c, d):
        assert x["block"] != x["next"] and {x["block"], x["next"]} == {0, 1}
    assert (a["end_block"], a["end_next"]) == (a["next"], a["block"])   # committed: swapped -- the next piece uses the block this one cleared
    assert b["block"] == a["next"]
    assert (b["end_block"], b["end_next"]) == (b["block"], b["next"])   # the parse launch failed: not committed ...
    assert c["block"] == b["block"] and c["next"] == b["next"]          # ... the call behind it sees the same block, which is still the cleared one
    assert len(b["epochs"]) == 1 and c["epochs"] == [b["epochs"][0] + 1, b["epochs"][0] + 2]   # (the epoch of the failed launch is spent)
    assert d["block"] == c["next"]
