#!/usr/bin/env python3
"""CPU model of the brute-force kernels' sample rounds (refill in kernels_path.hip, ticket_rounds in
rt_kernels.h), from the oracle's ray count per sample.

A wave takes tickets of 64 pixels (one 8x8 block) x `chunk` samples, opens a ticket's 64 items together
and closes them together.  A lane's sample of r rays takes r wave iterations.  Free-running, a lane
starts its next sample in the iteration after the last one ended, so a ticket takes max over lanes of
the sum over samples of r.  In rounds, no lane starts sample k + 1 before every lane has ended sample k,
so a ticket takes the sum over samples of the max over lanes.  The rule runs a wave's first ticket free
and every later one in rounds when the wave's previous ticket traced at least T x 64 x chunk x
(recursion + 1) rays (--all-miss: or at most 64 x chunk, the candidate that was not adopted).

Waves are modelled as runs of `--per-wave` consecutive chunks of one random block of the frame (the
dispenser deals a block's chunks next to each other).  Printed for each of the three: wave iterations,
the share of iterations in which some lane starts a sample, the share in which a lane is live and none
is below the recursion limit (shade returns before its body for the whole wave), and lane utilisation.

usage: tools/round_sim.py SCENE [--camera 0] [--size 1920x1080] [--chunk 11] [--tickets 96] [--per-wave 24]
                          [--per-block 0] [--hop 37] [--t 4/5] [--all-miss] [--seed 1] [--hit-only]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import OracleScene  # noqa: E402


def ticket_rays(orc, bx, by, s0, chunk, seed, W, H):
    """rays[lane, k] of the block's 64 pixels, samples s0 .. s0 + chunk - 1 (0 for a pixel off the frame)."""
    r = np.zeros((64, chunk), np.int64)
    for q in range(64):
        x, y = bx * 8 + (q & 7), by * 8 + (q >> 3)
        if x < W and y < H:
            for k in range(chunk):
                r[q, k] = orc.sample(x, y, seed, s0 + k)[2]
    return r


def run_ticket(r, rounds, limit):
    """(iterations, iterations with a sample start, iterations with every live lane at the limit, lane slots used)"""
    lanes, chunk = r.shape
    if rounds:
        longest = r.max(axis=0)
        iters = int(longest.sum())
        starts = int((longest > 0).sum())
        at_limit = int((longest == limit).sum())  # iteration `limit` of a round: only full-length paths are left
        return iters, starts, at_limit, int(r.sum())
    iters = int(r.sum(axis=1).max())
    start = np.zeros(iters + 1, bool)
    live = np.zeros(iters, np.int64)
    last = np.zeros(iters, np.int64)  # live lanes tracing ray number `limit` of their sample
    for q in range(lanes):
        t = 0
        for k in range(chunk):
            n = int(r[q, k])
            if n == 0:
                continue
            start[t] = True
            live[t:t + n] += 1
            if n == limit:
                last[t + n - 1] += 1
            t += n
    return iters, int(start[:iters].sum()), int(((live > 0) & (live == last)).sum()), int(r.sum())


def rule(prev_rays, chunk, recursion, num, den, all_miss=False):
    """ticket_rounds of rt_kernels.h for a later ticket of a wave (pool 64, RTCORE_SAMPLE_ROUNDS=1)"""
    samples = 64 * chunk
    return (all_miss and prev_rays <= samples) or prev_rays * den >= samples * (recursion + 1) * num


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--chunk", type=int, default=11, help="samples per item")
    ap.add_argument("--tickets", type=int, default=96)
    ap.add_argument("--per-wave", type=int, default=24,
                    help="consecutive tickets of one modelled wave (a block's chunks)")
    ap.add_argument("--per-block", type=int, default=0,
                    help="tickets a wave takes of one block before it moves on (0: it stays; a block's chunk count)")
    ap.add_argument("--hop", type=int, default=37, help="blocks, in row-major order, a wave moves on by")
    ap.add_argument("--all-miss", action="store_true",
                    help="the rule with the all-miss condition as well: rounds after a ticket of at most 64 x chunk rays")
    ap.add_argument("--t", default="4/5", help="the rule's T as a fraction NUM/DEN")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--hit-only", action="store_true", help="draw only blocks whose centre pixel's first sample hits")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    num, den = (int(v) for v in a.t.split("/"))
    path = a.scene
    if not os.path.exists(path):  # a scene of the package by its name
        import raytracercore_amd as rc

        path = rc.scene_path(a.scene)
    orc = OracleScene.from_file(path)
    orc.select_camera(a.camera)
    orc.set_size(W, H)
    recursion = orc.export()[0].recursion
    limit = recursion + 1
    rng = np.random.default_rng(a.seed)
    bxn, byn = (W + 7) // 8, (H + 7) // 8
    names = ("free", "rounds", "rule")
    tot = {n: np.zeros(4, np.int64) for n in names}
    hit_tickets = hit_rounds = room_tickets = room_rounds = rule_rounds = done = 0
    while done < a.tickets:
        bx, by = int(rng.integers(bxn)), int(rng.integers(byn))
        if a.hit_only and orc.sample(min(W - 1, bx * 8 + 4), min(H - 1, by * 8 + 4), a.seed, 0)[1]:
            continue
        prev = None
        blk = by * bxn + bx
        for i in range(min(a.per_wave, a.tickets - done)):
            c = i
            if a.per_block > 0:  # the wave moves along the dispenser's block order
                c = i % a.per_block
                b = (blk + (i // a.per_block) * a.hop) % (bxn * byn)
                bx, by = b % bxn, b // bxn
            r = ticket_rays(orc, bx, by, c * a.chunk, a.chunk, a.seed, W, H)
            rays = int(r.sum())
            in_rounds = prev is not None and rule(prev, a.chunk, recursion, num, den, a.all_miss)
            free, rnd = run_ticket(r, False, limit), run_ticket(r, True, limit)
            tot["free"] += free
            tot["rounds"] += rnd
            tot["rule"] += rnd if in_rounds else free
            hits = rays > int((r > 0).sum())  # some sample traced a second ray
            room = bool((r >= 2).any(axis=1).all())  # every pixel's paths bounce: the block lies in the room
            hit_tickets += hits
            hit_rounds += hits and in_rounds
            room_tickets += room
            room_rounds += room and in_rounds
            rule_rounds += in_rounds
            prev = rays
            done += 1
    print(f"{os.path.basename(path)} camera {a.camera} {W}x{H}, {a.chunk} samples per item, recursion {recursion}, "
          f"{done} tickets in runs of {a.per_wave}, T = {num}/{den}")
    base = tot["free"][0]
    for n in names:
        it, st, lim, used = (int(v) for v in tot[n])
        print(f"  {n:7s} wave iterations {it:8d} ({100.0 * (it - base) / base:+.2f} %)  with a sample start {100.0 * st / it:5.1f} %  "
              f"no lane below the limit {100.0 * lim / it:5.1f} %  lane utilisation {used / (64.0 * it):.3f}")
    print(f"  rule: {rule_rounds} of {done} tickets in rounds; {hit_rounds} of {hit_tickets} that hit anything; "
          f"{room_rounds} of {room_tickets} in-room tickets")


if __name__ == "__main__":
    main()
