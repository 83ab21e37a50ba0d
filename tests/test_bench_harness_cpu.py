"""bench.py's own rank fan-out: `--gpus N` without a launcher must start N ranks itself, before any GPU
call, and must refuse to report fewer ranks than requested.  No GPU here: TTV_BENCH_DRYRUN=1 runs the harness (spawn, rendezvous on
127.0.0.1, one gloo collective, rank 0's JSON line) without the measurement."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=300)


def test_gpus_2_spawns_two_ranks_and_reports_them():
    p = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], TTV_BENCH_DRYRUN="1")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks"]["world_size"] == 2 and line["dry_run"] is True and line["value"] is None


def test_gpus_beyond_the_visible_devices_is_refused():
    # no GPU in this container (and on a one-GPU box --gpus 2 must fail the same way): never a silent n_gpus: 1
    import torch
    if torch.cuda.device_count() >= 2:
        return
    p = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert p.returncode != 0
    assert "GPU(s) visible" in p.stderr and not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_world_size_mismatch_is_refused():
    p = _run(["--gpus", "4", "--steps", "1", "--warmup", "0"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", TTV_BENCH_DRYRUN="1")
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr


def test_train_dp_fan_out_hands_every_rank_the_same_run_token():
    """tools/train_dp.py --gpus N starts its own ranks; they meet at a shard directory named after the run token, so the token must be
    one per run, not one per rank."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_dp_tool", os.path.join(ROOT, "tools", "train_dp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    envs = mod.fan_out_envs(4, 29999)
    assert len({e["TTV_RUN_TOKEN"] for e in envs}) == 1
    assert [e["RANK"] for e in envs] == ["0", "1", "2", "3"] and all(e["WORLD_SIZE"] == "4" for e in envs)
    assert all(e["MASTER_ADDR"] == "127.0.0.1" and e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" for e in envs)


def test_steps_below_one_is_refused():
    p = _run(["--gpus", "1", "--steps", "0", "--warmup", "0"], TTV_BENCH_DRYRUN="1")
    assert p.returncode != 0 and "--steps 0" in p.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_the_whole_batch_when_it_fits(tmp_path):
    import numpy as np
    import torch
    bench = _bench_module()
    g = torch.Generator().manual_seed(3)
    recon = [torch.rand(3, 4, 8, 8, generator=g).to(torch.bfloat16) for _ in range(2)]
    idx = torch.randint(0, 4375, (2 * 5,), generator=g, dtype=torch.int32)
    shapes = bench.dump_outputs(str(tmp_path), recon, {"indices": idx})
    assert shapes == {"indices": [10], "recon": [2, 3, 4, 8, 8]}
    r, i = np.load(tmp_path / "recon.npy"), np.load(tmp_path / "indices.npy")
    assert r.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(r, torch.stack(recon).float().numpy()) and np.array_equal(i, idx.numpy().astype(np.float64))


def test_dump_outputs_samples_a_batch_beyond_the_budget_the_same_way_every_time(tmp_path, monkeypatch):
    import numpy as np
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    g = torch.Generator().manual_seed(4)
    recon = [torch.randn(3, 4, 32, 32, generator=g) for _ in range(3)]       # 147 kB as float32: over the budget
    idx = torch.arange(12, dtype=torch.int64)
    for d in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / d), recon, {"indices": idx})
        assert shapes == {"indices": [12], "recon_sample": [4096], "recon_sample_pos": [4096]}
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["indices.npy", "recon_sample.npy", "recon_sample_pos.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < (64 << 10) + 3 * 128     # + the .npy headers
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    pos = np.load(tmp_path / "a" / "recon_sample_pos.npy")
    assert pos.dtype == np.float64 and np.all(np.diff(pos) > 0) and pos[-1] < 3 * 3 * 4 * 32 * 32
    flat = torch.cat([r.reshape(-1) for r in recon]).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "recon_sample.npy"), flat[pos.astype(np.int64)])
