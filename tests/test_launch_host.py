"""sampler.devices on the host: device resolution, the rank launcher and its supervision, the launch decision of `jamun_sample`, a
two-rank gloo job started by the launcher, and a trajectory-writer error that must end every rank instead of leaving them in a
collective.  No GPU: the ranks are stub scripts or gloo processes with stub models."""
import datetime
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from jamun_amd import cmdline, dist
from jamun_amd import config as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
_LAUNCH_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", dist.LOCAL_DEVICES_ENV)


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in _LAUNCH_ENV}
    env["PYTHONPATH"] = os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p)
    env.update(extra)
    return env


def _no_count():
    raise AssertionError("the device count is only needed for -1")


# ---------------------------------------------------------------- resolve_devices

@pytest.mark.parametrize("devices,want", [
    (1, [0]), (3, [0, 1, 2]), ("2", [0, 1]), (-1, [0, 1, 2, 3]), ("-1", [0, 1, 2, 3]), ([0, 2], [0, 2]), ((1,), [1]), ([3], [3]),
    ("0,2", [0, 2]), ("[0,2]", [0, 2]), (" [0, 2] ", [0, 2]), ("[3]", [3]), ("1,", [1]), ("auto", None),
])
def test_resolve_devices_forms(devices, want):
    count = (lambda: 4) if devices in (-1, "-1") else _no_count
    assert dist.resolve_devices(devices, 1, count_devices=count) == want


@pytest.mark.parametrize("devices,match", [
    (0, "expected"), ("0", "expected"), (-2, "expected"), ([0, 0], "duplicate"), ("0,2,0", "duplicate"), ([-1], "negative"),
    ("[1,-3]", "negative"), ([], "expected"), (True, "expected"), ("gpu", "expected"), (1.5, "expected"), (None, "expected"),
    ([0, "1"], "expected"),
])
def test_resolve_devices_errors(devices, match):
    with pytest.raises(ValueError, match=match):
        dist.resolve_devices(devices, 1, count_devices=_no_count)


def test_resolve_devices_rejects_multi_node_and_an_empty_node():
    with pytest.raises(ValueError, match="multi-node launch is out of scope"):
        dist.resolve_devices(2, num_nodes=2, count_devices=_no_count)
    with pytest.raises(ValueError, match="no GPU is visible"):
        dist.resolve_devices(-1, 1, count_devices=lambda: 0)


def test_local_device_maps_local_rank_through_jamun_local_devices(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.delenv(dist.LOCAL_DEVICES_ENV, raising=False)
    assert dist.local_device() == torch.device("cuda", 1)  # unset: as before
    monkeypatch.setenv("LOCAL_RANK", "5")
    assert dist.local_device() == torch.device("cuda", 1)
    monkeypatch.setenv(dist.LOCAL_DEVICES_ENV, "0,2")
    monkeypatch.setenv("LOCAL_RANK", "1")
    assert dist.local_device() == torch.device("cuda", 2)
    monkeypatch.setenv(dist.LOCAL_DEVICES_ENV, "0,7")  # more devices asked for than are visible: a clear error, not a wrong GPU
    with pytest.raises(RuntimeError, match="no visible GPU for LOCAL_RANK 1"):
        dist.local_device()


# ---------------------------------------------------------------- launch_ranks on stub scripts

_STUB = r'''
import json, os, signal, sys, time
out, mode = sys.argv[1], sys.argv[2]
r = int(os.environ["RANK"])
keys = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "JAMUN_LOCAL_DEVICES")
with open(os.path.join(out, f"rank{r}.json"), "w") as f:
    json.dump(dict({k: os.environ.get(k) for k in keys}, pid=os.getpid()), f)
print(f"stdout-of-rank-{r}", flush=True)
if mode == "ok":
    sys.exit(0)
if mode == "fail" and r == 1:
    t0 = time.monotonic()
    while not os.path.exists(os.path.join(out, "rank0.json")) and time.monotonic() - t0 < 60:
        time.sleep(0.05)
    sys.stderr.write("x" * 6000 + "\nrank-1-failure-marker\n")
    sys.exit(3)
if mode == "stubborn" and r == 0:
    signal.signal(signal.SIGTERM, signal.SIG_IGN)
time.sleep(120)
'''


def _stub(tmp_path):
    script = tmp_path / "stub.py"
    script.write_text(_STUB)
    return [sys.executable, str(script), str(tmp_path)]


def _alive(pid: int) -> bool:
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    return True


def test_launch_ranks_all_ranks_succeed(tmp_path, capfd):
    rc = dist.launch_ranks(_stub(tmp_path) + ["ok"], [0, 2], timeout_s=120, env=_clean_env())
    assert rc == 0
    seen = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    for r, s in enumerate(seen):
        assert (s["RANK"], s["LOCAL_RANK"], s["WORLD_SIZE"], s["LOCAL_WORLD_SIZE"]) == (str(r), str(r), "2", "2")
        assert s["JAMUN_LOCAL_DEVICES"] == "0,2" and s["MASTER_ADDR"] == "127.0.0.1"
    assert seen[0]["MASTER_PORT"] == seen[1]["MASTER_PORT"] and int(seen[0]["MASTER_PORT"]) > 0
    out = capfd.readouterr().out
    assert "stdout-of-rank-0" in out and "stdout-of-rank-1" not in out  # rank 0's stdout is relayed, the others' is not


def test_launch_ranks_ends_the_job_at_the_first_failure(tmp_path, capfd):
    t0 = time.monotonic()
    rc = dist.launch_ranks(_stub(tmp_path) + ["fail"], [0, 1], env=_clean_env())
    dt = time.monotonic() - t0
    assert rc == 3
    assert dt < 15, dt
    assert not _alive(json.load(open(tmp_path / "rank0.json"))["pid"])  # rank 0 was sleeping for 120 s: it was terminated
    err = capfd.readouterr().err
    assert "rank 1 (GPU 1) exited with code 3" in err and "rank-1-failure-marker" in err
    assert "x" * 4096 not in err  # only the tail of the failed rank's stderr


def test_launch_ranks_timeout_returns_124_and_kills_a_rank_that_ignores_sigterm(tmp_path, capfd):
    t0 = time.monotonic()
    rc = dist.launch_ranks(_stub(tmp_path) + ["stubborn"], [0, 1], timeout_s=1.0, env=_clean_env())
    dt = time.monotonic() - t0
    assert rc == 124
    assert dt < 25, dt
    for r in range(2):
        assert not _alive(json.load(open(tmp_path / f"rank{r}.json"))["pid"])
    assert "timeout" in capfd.readouterr().err


# ---------------------------------------------------------------- Sampler(devices=...) outside a launched job

def test_sampler_refuses_several_devices_outside_a_launch(monkeypatch):
    from jamun_amd.sampling import Sampler

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for devices in (2, "0,1", [0, 3]):
        with pytest.raises(RuntimeError) as e:
            Sampler(devices=devices)
        for name in ("jamun_sample", "jamun_amd.dist.launch_ranks", "torch.distributed.run"):
            assert name in str(e.value)
    with pytest.raises(ValueError):
        Sampler(devices=0)
    Sampler(devices=1)
    Sampler(devices="auto")
    Sampler()
    monkeypatch.setenv("WORLD_SIZE", "1")  # inside a launched job devices is not enforced (torchrun configs say devices: 1)
    monkeypatch.setenv("RANK", "0")
    Sampler(devices=2)


# ---------------------------------------------------------------- the launch decision of jamun_sample

def _argv(*extra):
    return ["--config-dir=" + CONFIGS, "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=ckpts", *extra]


def test_launch_plan_decides_on_the_composed_config(tmp_path):
    for extra in ((), ("sampler.devices=1",), ("++sampler.devices=auto",), ("sampler.devices=[1]",)):
        argv = _argv(*extra)
        assert cmdline.launch_plan(cmdline.compose(argv, str(tmp_path)), argv, environ={}) is None, extra
    argv = _argv("sampler.devices=2")
    cfg = cmdline.compose(argv, str(tmp_path))
    assert cmdline.launch_plan(cfg, argv, environ={"WORLD_SIZE": "2"}) is None  # a rank of a launched job does not launch again
    devices, cmd = cmdline.launch_plan(cfg, argv, environ={})
    assert devices == [0, 1]
    assert cmd[:3] == [sys.executable, "-m", "jamun_amd.cmdline"] and cmd[3:-1] == argv
    m = re.fullmatch(r'\+\+run_key="(.*)"', cmd[-1])
    assert m and re.fullmatch(r"\d{4}-\d\d-\d\d_\d\d-\d\d-\d\d", m.group(1)), cmd[-1]
    # every rank resolves the same run_key, whenever it starts
    for now in (datetime.datetime(2001, 2, 3, 4, 5, 6), datetime.datetime(2030, 1, 1)):
        assert C.resolve(cmdline.compose(cmd[3:], str(tmp_path)), now=now)["run_key"] == m.group(1)
    devices, cmd = cmdline.launch_plan(cmdline.compose(_argv("sampler.devices=[0,2]", "run_key=mine"), str(tmp_path)), _argv(), environ={})
    assert devices == [0, 2] and cmd[-1] == '++run_key="mine"'
    with pytest.raises(ValueError, match="multi-node"):
        cmdline.launch_plan(cmdline.compose(_argv("sampler.devices=2", "++sampler.num_nodes=2"), str(tmp_path)), [], environ={})


# ---------------------------------------------------------------- a two-rank gloo job started by launch_ranks

_COMMON = r'''
import json, os, sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from jamun_amd import cmdline, dist, synth
from jamun_amd import config as C
from jamun_amd.callbacks import SaveTrajectoryCallback
from jamun_amd.data import WalkerBatch
from jamun_amd.sampling import Sampler
dist.local_device = lambda: torch.device("cpu")  # the host path this test is about, also where a GPU is visible (the stubs live on the CPU)
MOL = synth.random_chain(6, seed=0)
class DS:
    molecule = dict(MOL)
    def label(self): return "m"
class StubModel:
    device = torch.device("cpu")
    def to(self, d): return self
    def eval(self): return self
class StubBatchSampler:
    sigma = 0.04
    mcmc = type("M", (), {"rng": "philox"})()
    def __init__(self, pause=0.0): self.pause = pause
    def sample(self, model, y_init, v_init):
        time.sleep(self.pause)
        T, rank = 3, dist.rank_world()[0]
        xt = y_init[None].repeat(T, 1, 1) + 0.01 * torch.randn(T, y_init.shape[0], 3) + 100.0 * rank  # seed + rank stream; rank mark
        return {"xhat": y_init, "y": y_init, "v": torch.zeros_like(y_init), "sample": y_init, "xhat_traj": xt, "y_traj": xt.clone(),
                "score_traj": xt.clone(), "t_traj": torch.ones(T)}
'''

_LAUNCHED = _COMMON + r'''
argv = sys.argv[2:]  # jamun_sample's command line, as launch_plan hands it to every rank
cfg = cmdline.compose(argv)
rank, world = dist.init_process_group("gloo")
head = C.resolve({k: cfg[k] for k in ("paths", "task_name", "run_group", "run_key")})
run_dir = head["paths"]["run_path"]
os.makedirs(run_dir, exist_ok=True)
os.chdir(run_dir)
smp_cfg = C.resolve(cfg)["sampler"]
cb = SaveTrajectoryCallback([DS()], output_dir="sampler", write_pdb=False)
sampler = Sampler(devices=smp_cfg["devices"], callbacks=[cb], shard_walkers=bool(smp_cfg.get("shard_walkers", False)))
torch.manual_seed(cfg["seed"] + sampler.fabric.global_rank)
sampler.sample(model=StubModel(), batch_sampler=StubBatchSampler(), num_batches=2, init_graphs=WalkerBatch.from_molecules([MOL] * 3, labels=["m"] * 3))
keys = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "JAMUN_LOCAL_DEVICES")
json.dump({"world": world, "env": {k: os.environ[k] for k in keys}}, open(f"rank{rank}.json", "w"))
dist.barrier()
torch.distributed.destroy_process_group()
'''


def _launched_job(tmp_path, *extra):
    argv = _argv("sampler.devices=2", *extra)
    devices, cmd = cmdline.launch_plan(cmdline.compose(argv, str(tmp_path)), argv, environ={})
    script = tmp_path / "launched.py"
    script.write_text(_LAUNCHED)
    rc = dist.launch_ranks([sys.executable, str(script), ROOT] + cmd[3:], devices, timeout_s=240, env=_clean_env(JAMUN_ROOT_PATH=str(tmp_path)))
    assert rc == 0
    runs = tmp_path / "outputs" / "sample" / "dev" / "runs"
    assert len(os.listdir(runs)) == 1  # one run directory for both ranks
    run_dir = runs / os.listdir(runs)[0]
    for r in range(2):
        seen = json.load(open(run_dir / f"rank{r}.json"))
        assert seen["world"] == 2 and seen["env"] == {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "2", "JAMUN_LOCAL_DEVICES": "0,1"}
    npy = run_dir / "sampler" / "m" / "predicted_samples" / "npy"
    return {f[:-4]: np.load(npy / f) for f in os.listdir(npy)}


def test_launched_gloo_job_replicates_walkers_per_rank(tmp_path):
    files = _launched_job(tmp_path)
    assert sorted(files) == sorted([str(i) for i in range(12)] + ["joined"])  # 2 ranks x 3 walkers x 2 batches
    assert files["joined"].shape == (6, 12 * 3, 3)
    # rank-major within each batch: chains 0-2 from rank 0, 3-5 from rank 1, then the second batch
    assert [int(files[str(i)].mean() // 50) for i in range(12)] == [0, 0, 0, 2, 2, 2, 0, 0, 0, 2, 2, 2]
    for i in range(3):  # seed + rank: rank 1's chains are not rank 0's shifted
        d = files[str(i + 3)] - 100.0 - files[str(i)]
        assert np.abs(d).max() > 1e-3


def test_launched_gloo_job_shards_walkers(tmp_path):
    files = _launched_job(tmp_path, "++sampler.shard_walkers=true")
    assert sorted(files) == sorted([str(i) for i in range(6)] + ["joined"])  # 3 walkers split over 2 ranks, 2 batches
    assert [int(files[str(i)].mean() // 50) for i in range(6)] == [0, 0, 2, 0, 0, 2]


# ---------------------------------------------------------------- a writer error on rank 0 ends both ranks

_WRITER_ERROR = _COMMON + r'''
class FailingWriter(SaveTrajectoryCallback):
    def _write_batch(self, label, blocks, start):
        raise OSError("writer-failure-marker: no space left on device")
rank, world = dist.init_process_group("gloo")
cb = FailingWriter([DS()], output_dir=os.path.join(sys.argv[2], "sampler"), write_pdb=False, async_write=sys.argv[3] == "async")
sampler = Sampler(callbacks=[cb])
torch.manual_seed(42 + rank)
sampler.sample(model=StubModel(), batch_sampler=StubBatchSampler(pause=0.3), num_batches=4, init_graphs=WalkerBatch.from_molecules([MOL] * 2, labels=["m"] * 2))
print("finished sampling")
'''


@pytest.mark.parametrize("mode", ["async", "sync"])
def test_writer_error_on_rank_0_ends_every_rank_with_its_message(tmp_path, mode):
    script = tmp_path / "writer_error.py"
    script.write_text(_WRITER_ERROR)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = _clean_env(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path), mode], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=120) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, (o, e)) in enumerate(zip(procs, outs)):
        assert p.returncode not in (0, None), (r, e[-2000:])
        assert "finished sampling" not in o
        assert "writer-failure-marker" in e, (r, e[-2000:])
    assert "OSError: writer-failure-marker" in outs[0][1]
    assert "RuntimeError: rank 0 failed: OSError: writer-failure-marker" in outs[1][1]
