"""Diagnostic: what overlapping consecutive path-kernel launches could save, priced without a library change.

Two GpuRaytracer objects over the same scene, camera and traversal (each owns its partials, dispensers,
start rows and events), each on its own non-default torch stream with its own accumulators, render
alternate steps A, B, A, B ... for 2N steps with one sync at the end; launch k+1's path kernel can then
enter the SIMDs that launch k's last waves leave.  Against it: 2N steps of one object on one stream, the
same call (bench.py's step: zero the slot, rt_render_bands_device of the whole frame).  Three alternating
rounds after a warm-up; the single-stream rounds' fastest-to-slowest range is the spread the saving is
held against.
With `pick`, object B's stream is the first of eight fresh torch streams on which a short operation finishes
while a long one still runs on A's stream: two HIP streams can share one hardware queue, and then run in
submission order whatever their events allow.
usage: python tools/launch_overlap_pricing.py [config] [N] [pick]     (config: a bench.py config, default bounce1080)"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch

import bench
import raytracercore_amd as rc
from raytracercore_amd import sharding

cfg = sys.argv[1] if len(sys.argv) > 1 else "bounce1080"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
pick = len(sys.argv) > 3 and sys.argv[3] == "pick"
scene_file, cam, W, H, spp = bench.CONFIGS[cfg]
scene = bench.load_scene(rc, scene_file)
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
plane = sharding.slot_rows(H, 1, sharding.BAND) * W


class Side:
    def __init__(self):
        self.gpu = rc.GpuRaytracer(scene, cam, device=0, size=(W, H))
        self.stream = torch.cuda.Stream(dev)
        self.slots = [torch.zeros(4 * plane, dtype=torch.float64, device=dev) for _ in range(2)]
        self.rays = torch.zeros(1, dtype=torch.int64, device=dev)
        self.k = 0

    def step(self, sample_k):
        slot = self.slots[self.k % 2]
        self.k += 1
        with torch.cuda.stream(self.stream):
            slot.zero_()
            s_, n_, m_ = sharding.slot_views(slot, plane)
            self.gpu.render_bands_device(sharding.BAND, 1, 0, spp, 0, sample_k * spp, s_.data_ptr(), n_.data_ptr(),
                                         m_.data_ptr(), plane, self.rays.data_ptr(), self.stream.cuda_stream)


def concurrent(sx, sy):
    """True when a short operation on sy finishes while a long one queued before it on sx still runs."""
    t = torch.zeros(64, device=dev)
    ex, ey = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(sx):
        torch.cuda._sleep(100_000_000)  # tens of ms
        ex.record(sx)
    with torch.cuda.stream(sy):
        t.zero_()
        ey.record(sy)
    ey.synchronize()
    ran_beside = not ex.query()
    torch.cuda.synchronize(dev)
    return ran_beside


a, b = Side(), Side()
if pick:
    pool = [b.stream] + [torch.cuda.Stream(dev) for _ in range(8)]
    beside = [concurrent(a.stream, s) for s in pool]
    print("streams that run beside A's (B's own first):", beside, flush=True)
    if any(beside):
        b.stream = pool[beside.index(True)]
    else:
        print("no stream ran beside A's: every pair shares a hardware queue", flush=True)


def single(first):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(2 * N):
        a.step(first + k)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (2 * N) * 1e3


def dual(first):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(2 * N):
        (a if k % 2 == 0 else b).step(first + k)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / (2 * N) * 1e3


single(0)
dual(0)
ones, twos = [], []
for r in range(3):
    ones.append(single((2 * r + 1) * 2 * N))
    twos.append(dual((2 * r + 2) * 2 * N))
    print(f"round {r}: one object, one stream {ones[-1]:.4f} ms/step   two objects, two streams {twos[-1]:.4f} ms/step",
          flush=True)
spread = max(ones) - min(ones)
saving = min(ones) - max(twos)
print(f"{cfg} x {2 * N} steps: single {min(ones):.4f}-{max(ones):.4f} (spread {spread:.4f}), dual "
      f"{min(twos):.4f}-{max(twos):.4f}; saving (fastest single - slowest dual) {saving:.4f} ms/step = "
      f"{saving / min(ones) * 100:.2f} % = {saving / spread if spread > 0 else float('inf'):.1f} spreads", flush=True)
ka = a.gpu.kernel_times(min(N, 64))
print(f"kernel ms (object A, last {len(ka)} launches, overlapped event pairs): min {min(ka):.3f} max {max(ka):.3f}", flush=True)
a.gpu.close()
b.gpu.close()
