"""The depth of CG's ring of directions as a pure function of byte counts (csrc/mk_ringdepth.h): what a set-up with
MK_CG_XDEFER unset asks for.  A host program that includes only that header.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB, GIB = 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("ringdepth") / "ringdepth_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "ringdepth_main.cpp"), "-o", exe],
                   check=True, timeout=120)
    return exe


def rule(program, cases):
    """[(depth, fit)] of the cases (vector bytes, free bytes, buffers held, cap)"""
    p = subprocess.run([program] + ["%d:%d:%d:%d" % c for c in cases], capture_output=True, text=True, check=True, timeout=5)
    lines = p.stdout.splitlines()
    assert lines[0] == "max 32 min_bytes %d" % (256 * MIB)
    return [tuple(int(t) for t in l.split()) for l in lines[1:]]


def by_hand(vec, free, held, cap):
    """The rule restated: every buffer beyond the first two is an extra; all extras together may take an eighth of what was free
    before the first of them (the extras held already are not free any more: they are added back)."""
    if vec <= 256 * MIB:
        return 1
    budget = (free + max(held - 2, 0) * vec) // 8
    return min(1 + budget // vec, cap or 32, 32)


def test_the_cases_of_the_rule(program):
    cases = [
        (256 * MIB, 280 * 10 ** 9, 2, 0),                     # a vector that stays in the Infinity Cache: nothing to defer for
        (GIB, 280 * 10 ** 9, 2, 0),                           # 512^3 on a 288 GB device: the cap, 31 vectors beyond the pair
        (GIB, 40 * GIB, 2, 0),                                # an eighth of 40 GiB holds five extras: m = 6
        (GIB, 280 * 10 ** 9, 2, 8),                           # the caller's bound (a placement probe)
        (GIB, 0, 2, 0),                                       # nothing free: the pair
        (GIB, 0, 0, 0),
        (256 * MIB + 8, 280 * 10 ** 9, 1, 0),                 # one entry beyond the threshold
    ]
    got = rule(program, cases)
    assert [d for d, _ in got] == [1, 32, 6, 8, 1, 1, 32]
    assert [d for d, _ in got] == [by_hand(*c) for c in cases]


def test_held_buffers_are_added_back_and_the_rule_is_monotone(program):
    # a ring that holds 9 buffers (a probe's) asks again: what it holds counts as free, so the answer is that of the first call
    # made with the 7 extras still unallocated
    first = rule(program, [(GIB, 100 * GIB, 2, 0)])[0]
    again = rule(program, [(GIB, 100 * GIB - 7 * GIB, 9, 0)])[0]
    assert first == again == (13, 13)
    frees = [k * GIB for k in range(0, 300, 7)]
    for vec in (GIB, 3 * GIB + 8, 257 * MIB):
        got = rule(program, [(vec, f, 2, 0) for f in frees])
        depths = [d for d, _ in got]
        assert depths == sorted(depths) and depths[0] == 1 and all(1 <= d <= 32 for d in depths)
        assert depths == [by_hand(vec, f, 2, 0) for f in frees]
        for cap in (1, 8, 31, 32, 0, 40, -3):                  # (a cap outside 1 .. 32 is no cap)
            capped = [d for d, _ in rule(program, [(vec, f, 2, cap) for f in frees])]
            top = cap if 1 <= cap <= 32 else 32
            assert capped == [min(d, top) for d in depths]


def test_sizes_beyond_32_bits_and_a_full_address_space(program):
    big = (1 << 64) - 1
    cases = [(5 * GIB, big, 2, 0), (5 * GIB, big, 33, 0), (big, big, 2, 0), (big // 2, big, 40, 0), (3 * GIB, 100 * GIB + 5, 2, 0)]
    got = rule(program, cases)
    assert [d for d, _ in got] == [32, 32, 1, 6, 5] == [by_hand(*c) for c in cases]
