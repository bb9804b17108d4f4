"""bench.py's launch contract on the CPU (no GPU needed): `--gpus N` without a launcher starts
N rank processes instead of measuring one GPU and calling it N, and a launcher world that
disagrees with --gpus is refused.  Here the ranks fail (no device), so the run must fail too --
never exit 0 with an `n_gpus: 1` line."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--steps", "1", "--warmup", "0", "--spp", "1", "--config", "bounce256", "--no-cpu-baseline"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = env.get("HIP_VISIBLE_DEVICES", "")
    env.update(kw)
    return env


def test_gpus2_without_launcher_is_not_one_gpu():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + ARGS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert '"n_gpus": 1' not in r.stdout
    if r.returncode == 0:  # only possible where two devices exist: then it measured two
        assert '"n_gpus": 2' in r.stdout


def test_dump_outputs_samples_a_large_frame_within_the_budget(tmp_path):
    """--dump-outputs' writer: a frame whose arrays pass the budget is written as one fixed, seeded
    sample of its pixels (the same for every array and from run to run), in float64, under 64 MB."""
    import numpy as np

    import bench

    npix = 1920 * 1080
    arrays = {"frame_sum": np.arange(3 * npix, dtype=np.float64).reshape(3, npix),
              "frame_samples": np.arange(npix, dtype=np.int64), "frame_misses": np.zeros(npix, np.int32),
              "step_sum": np.ones((3, npix)), "step_samples": np.arange(npix, dtype=np.int32),
              "step_misses": np.zeros(npix, np.int32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, {"rays": 12345})
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted([k + ".npy" for k in arrays] + ["pixel_index.npy", "rays.npy"])
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 * 10 ** 6
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["pixel_index"].astype(np.int64)
    assert 0 < idx.size < npix and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < npix
    assert idx.size * 11 * 8 > 50 * 10 ** 6  # the budget is used, not a token sample
    assert np.array_equal(got["frame_samples"], idx) and np.array_equal(got["step_samples"], idx)
    assert np.array_equal(got["frame_sum"], arrays["frame_sum"][:, idx]) and got["rays"][0] == 12345
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f)), f
    # a small frame is written whole
    bench.dump_outputs(str(tmp_path / "c"), {"x": np.arange(10, dtype=np.int32)}, {})
    assert np.array_equal(np.load(tmp_path / "c" / "pixel_index.npy"), np.arange(10))
    assert np.array_equal(np.load(tmp_path / "c" / "x.npy"), np.arange(10))


def test_world_size_mismatch_refused():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + ARGS, cwd=ROOT,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr and '"n_gpus"' not in r.stdout
