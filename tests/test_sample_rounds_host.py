"""The sample rounds' rule on the host (ticket_rounds in rt_kernels.h, the function the kernels call)
and the launch record's field, from a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer (`make rounds_rule_check_asan`, tests/host/rounds_rule_check.cpp).

The rule, restated here with exact fractions: RTCORE_SAMPLE_ROUNDS=0 never, 2 always; 1: a wave's first
ticket runs free, a later one in rounds when the previous ticket traced at least T x pool x chunk x
(recursion + 1) rays, T = 4/5; a ticket whose samples all missed (pool x chunk rays) is followed by a free
one.  Edges: first ticket, all-miss and one ray either side of it, one ray either side of T, a short last
ticket, recursion 0, the largest ticket.
"""
import os
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracercore_amd", "csrc")
T = Fraction(4, 5)


@pytest.fixture(scope="module")
def lines():
    subprocess.run(["make", "-s", "-C", CSRC, "rounds_rule_check_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("RTCORE_SAMPLE_ROUNDS", None)
    out = subprocess.run([os.path.join(CSRC, "_obj_asan", "rounds_rule_check")], capture_output=True, text=True, env=env,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return [ln.split() for ln in out.stdout.splitlines() if ln]


def _expected(mode, pool, chunk, recursion, first, prev):
    if mode != 1:
        return mode == 2
    if first:
        return False
    samples = pool * chunk
    return Fraction(prev) >= T * samples * (recursion + 1)


def test_rule_at_its_edges(lines):
    rows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "rule"]
    assert len(rows) >= 6 * 3 * 2 * 8
    seen = set()
    for mode, pool, chunk, recursion, first, prev, got in rows:
        assert bool(got) == _expected(mode, pool, chunk, recursion, bool(first), prev), (mode, pool, chunk, recursion, first, prev)
        if mode == 1 and not first:
            seen.add((recursion == 0, bool(got)))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_named_cases(lines):
    got = {tuple(int(v) for v in ln[1:7]): bool(int(ln[7])) for ln in lines if ln[0] == "rule"}
    full = 64 * 11 * 11  # C2's ticket: 64 items of 11 samples, recursion 10
    at_t = -(-full * 4 // 5)
    assert got[(1, 64, 11, 10, 1, full)] is False         # a wave's first ticket
    assert got[(1, 64, 11, 10, 0, 64 * 11)] is False      # all-miss: one ray per sample
    assert got[(1, 64, 11, 10, 0, 0)] is False            # a ticket of closed items
    assert got[(1, 64, 11, 10, 0, at_t - 1)] is False     # just below T
    assert got[(1, 64, 11, 10, 0, at_t)] is True          # at T
    assert got[(1, 64, 11, 10, 0, 64 * 7 * 11)] is False  # after a short last ticket of 7 samples: 7/11 < T
    assert got[(1, 64, 64, 0, 0, 64 * 64)] is True        # recursion 0: every sample is one ray
    assert got[(1, 64, 64, 0, 0, 1)] is False


def test_launch_field(lines):
    modes = {(ln[1], int(ln[2])): int(ln[3]) for ln in lines if ln[0] == "mode"}
    for kernel in range(4):
        assert modes[("-", kernel)] == 1 and modes[("empty", kernel)] == 0
        assert [modes[(s, kernel)] for s in ("0", "1", "2", "7", "-3")] == [0, 1, 2, 2, 0]
    size, off, bound, cull = (int(v) for v in next(ln for ln in lines if ln[0] == "size")[1:])
    # the field lies in what was padding between scene_bound and the record's last pointer
    assert off == bound + 4 and cull == bound + 8 and size == cull + 8
