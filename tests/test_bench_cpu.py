"""bench.py's host-side pieces without a GPU: the CPU baseline leg (the oracle on host cores, a tiny
sample here), the algorithmic-bytes model the roofline uses, and the committed PMC traffic lookup."""
import bench
from lsm.perf_model import step_bytes


def test_cpu_baseline_leg_small_sample():
    c = bench.CONFIGS[2]   # filter off: no HJ table needed
    args = bench.make_args(c)
    r = bench.cpu_baseline(args, None, None, ep=4, cores=2, envs_per_worker=1, steps=3)
    assert set(r) == {"value", "unit", "cores", "kind", "sample"}
    assert r["value"] > 0 and r["cores"] == 2 and r["kind"] == "port" and r["unit"] == "agent-steps/s"


def test_step_bytes_model():
    """record (read whole, hot part written) + outputs + HJ gathers (64 B per ordered
    agent pair + 256 B per ego for the 4-D table)."""
    d = step_bytes(8, 2, "double_integrator", True, "reference")
    assert d["gather_bytes"] == 64 * 8 * 7 + 256 * 8 == 5632 and not d["block"]
    assert d["hbm_bytes"] == d["state"] + d["outputs"] + d["gather_bytes"] == 37465   # state incl. actions
    assert step_bytes(8, 2, "double_integrator", False)["gather_bytes"] == 0
    d = step_bytes(64, 2, "double_integrator", True, "compact")
    assert d["block"] and d["E"] == 192 and d["hbm_bytes"] == 955409
    d = step_bytes(16, 2, "airtaxi", True, "reference")
    assert d["gather_bytes"] == 128 * 16 * 15 + 32 * 32 * 16


def test_timed_window_straddles_an_episode_boundary():
    for w, k, epl in ((5, 20, 250), (250, 1000, 250), (0, 1, 350), (3, 7, 10), (100, 2, 250)):
        pre = bench.timed_window(w, k, epl)
        assert pre >= w
        boundaries = [t for t in range(pre, pre + k) if (t + 1) % epl == 0]
        assert boundaries or k < 2, (w, k, epl, pre)


def _fake_env(n, N=3, E=5, compact=False):
    """Host tensors with the shapes and dtypes of GpuGraphVecEnv's outputs (values: a running index)."""
    import types
    import torch
    fill = lambda shape, dt: torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float64).reshape(shape).to(dt)
    e = types.SimpleNamespace(E=E, t_obs=fill((n, N, 6), torch.float32), agent_id=fill((n, N, 1), torch.int64),
                              t_node=fill((n, N, E, 7), torch.float32), t_rew=fill((n, N), torch.float32),
                              t_done=fill((n, N), torch.float64) % 2 == 1, t_info=fill((n, N, 4), torch.float64),
                              t_reset=fill((n,), torch.float64) % 3 == 0, t_epinfo=fill((n, 8), torch.float64),
                              t_state=fill((n, N, 4), torch.float64))
    e.t_adj = fill((n, E, E) if compact else (n, N, E, E), torch.float32)
    e.t_adj_mask = torch.full((n, N, 1), 0b10010, dtype=torch.int64) if compact else None
    return e


def test_dump_outputs_names_dtypes_and_values(tmp_path):
    """--dump-outputs: one .npy per output of the step, float64 outputs as float64 and every other
    dtype as float32, values unchanged; a compact adjacency's mask words unpacked to 0/1 per entity."""
    import numpy as np
    env = _fake_env(4, compact=True)
    info = bench.dump_outputs(str(tmp_path), bench.step_outputs(env, None), 4, 0, 1)
    assert info["envs"] == info["of"] == 4
    names = {"obs", "agent_id", "node_obs", "adj", "adj_mask", "rewards", "dones", "info", "reset", "ep_info", "state"}
    assert set(info["arrays"]) == names == {p.name[:-4] for p in tmp_path.iterdir()}
    got = {k: np.load(tmp_path / (k + ".npy")) for k in names}
    for k in ("info", "ep_info", "state"):
        assert got[k].dtype == np.float64
    for k in names - {"info", "ep_info", "state"}:
        assert got[k].dtype == np.float32, k
    np.testing.assert_array_equal(got["obs"], env.t_obs.numpy())
    np.testing.assert_array_equal(got["state"], env.t_state.numpy())
    np.testing.assert_array_equal(got["dones"], env.t_done.numpy().astype(np.float32))
    assert got["adj_mask"].shape == (4, 3, 5) and (got["adj_mask"] == [0, 1, 0, 0, 1]).all()


def test_dump_outputs_files_are_finite_and_keep_the_nonfinite_entries(tmp_path):
    """The info rows hold +inf for agents that are done: every file written is finite, the entry is 0
    in info.npy and its kind (1 +inf, 2 -inf, 3 NaN) stands in info_nonfinite.npy; arrays without
    such entries get no such file."""
    import numpy as np
    env = _fake_env(4)
    env.t_info[1, 2, 1] = float("inf")
    env.t_info[3, 0, 1] = float("-inf")
    env.t_info[0, 0, 3] = float("nan")
    want = env.t_info.numpy().copy()
    info = bench.dump_outputs(str(tmp_path), bench.step_outputs(env, None), 4, 0, 1)
    assert info["nonfinite_entries"] == {"info": 3} and "info_nonfinite" in info["arrays"]
    assert {p.name[:-4] for p in tmp_path.iterdir()} == set(info["arrays"])
    assert [p.name for p in tmp_path.iterdir() if "nonfinite" in p.name] == ["info_nonfinite.npy"]
    for p in tmp_path.iterdir():
        assert np.isfinite(np.load(p)).all(), p.name
    got, code = np.load(tmp_path / "info.npy"), np.load(tmp_path / "info_nonfinite.npy")
    assert code.dtype == np.float32 and code.shape == got.shape and got.dtype == np.float64
    assert (code[1, 2, 1], code[3, 0, 1], code[0, 0, 3], code.sum()) == (1, 2, 3, 6)
    assert (got[code != 0] == 0).all()
    np.testing.assert_array_equal(got[code == 0], want[code == 0])


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    """Outputs larger than the budget: every array keeps the same sorted, seeded sample of envs (the
    same from call to call), and the files together stay within the budget; ranks share it."""
    import numpy as np
    env = _fake_env(64)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), bench.step_outputs(env, None), 64, 0, 1)
    bench.dump_outputs(str(b), bench.step_outputs(env, None), 64, 0, 1)
    assert 1 <= info["envs"] < 64 and info["of"] == 64
    assert sum(p.stat().st_size for p in a.iterdir()) <= 20000
    for p in a.iterdir():
        np.testing.assert_array_equal(np.load(p), np.load(b / p.name))
    rows = np.load(a / "ep_info.npy")[:, 0] / 8          # ep_info[e, 0] = 8 e: the envs kept
    assert len(rows) == info["envs"] and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(np.load(a / "state.npy"), env.t_state.numpy()[rows.astype(int)])
    half = bench.dump_outputs(str(tmp_path / "c"), bench.step_outputs(env, None), 64, 1, 2)
    assert half["envs"] <= info["envs"] // 2 + 1
    assert all(p.name.endswith(".rank1.npy") for p in (tmp_path / "c").iterdir())


def test_multi_rank_launch_dry_run():
    """bench.py --gpus 2 starts two rank processes itself (no torchrun): each sees WORLD_SIZE=2, owns
    the env block [r * n, (r + 1) * n) and joins the episode-summary collective (gloo here)."""
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, bench.__file__, "--gpus", "2", "--dry-run", "--envs", "8",
                          "--steps", "20", "--warmup", "5"], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["world_size"] == 2
    assert [(r["rank"], r["env_offset"], r["envs"]) for r in line["ranks"]] == [(0, 0, 8), (1, 8, 8)]
    assert line["max_over_ranks"] == 2.0
    # mean over both ranks' 16 envs of arange rows
    assert line["episode_summary"]["travel_time_mean"] == 60.0
    assert line["untimed_steps"] == 240


def test_world_size_must_match_gpus():
    import os
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, bench.__file__, "--gpus", "2", "--dry-run"], capture_output=True,
                         text=True, timeout=120, env=env)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def test_traffic_lookup_matches_workload_and_build():
    import json
    import os
    p = os.path.join(os.path.dirname(bench.__file__), "profiles", "pmc_traffic.json")
    e = json.load(open(p)).get("config3", {})
    bid = e.get("build_id")
    if bid:
        assert bench.load_traffic(3, e["num_envs"], bid) > 1e8
    assert bench.load_traffic(3, 123, bid) is None       # a different workload never borrows the number
    assert bench.load_traffic(3, 4096, "not-this-build") is None   # nor a different library build
