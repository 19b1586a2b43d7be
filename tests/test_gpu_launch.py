"""GPU tests of sampler.devices through `jamun_sample`: one device selected in-process writes what a run without the key writes, bit
for bit; with two visible GPUs, `sampler.devices=2` starts two ranks (one per GPU) that write into one run directory.  Every run is
a subprocess under a time limit; run with -x so that the module stops at the first failure."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKERS, STEPS, BATCHES = 4, 20, 2


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from jamun_amd import pdb, synth

    tmp = tmp_path_factory.mktemp("launch")
    mol = dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)
    pdb_path = str(tmp / "uncapped_AG.pdb")
    pdb.write_pdb(pdb_path, mol, mol["pos"][None])
    ck_dir = tmp / "ckpt"
    ck_dir.mkdir()
    torch.save(synth.synthetic_checkpoint(output_gain=0.05, prefix="g._orig_mod."), str(ck_dir / "epoch=7-step=100.ckpt"))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                            "JAMUN_LOCAL_DEVICES")}
    env.update(JAMUN_ROOT_PATH=str(tmp), PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    base = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", f"++init_pdbs=[{pdb_path}]", f"++checkpoint_dir={ck_dir}",
            "checkpoint_type=best_so_far", f"num_sampling_steps_per_batch={STEPS}", f"repeat_init_samples={WALKERS}", f"num_batches={BATCHES}"]

    def run(run_key, *extra, timeout=300, launch_on=None):
        """jamun_sample as a user runs it (or, with ``launch_on``, as the ranks of dist.launch_ranks on those GPUs); returns the run's
        files under sampler/uncapped_AG (relative path -> bytes)."""
        cmd = [sys.executable, "-m", "jamun_amd.cmdline", *base, f"run_key={run_key}", *extra]
        if launch_on is None:
            r = subprocess.run(cmd, cwd=str(tmp), env=env, capture_output=True, text=True, timeout=timeout)
            assert r.returncode == 0, r.stderr[-3000:]
        else:
            from jamun_amd import dist

            assert dist.launch_ranks(cmd, launch_on, timeout_s=timeout, env=env) == 0  # (every path in cmd and env is absolute)
        runs = tmp / "outputs" / "sample" / "dev" / "runs"
        assert os.path.isdir(runs / run_key), (run_key, os.listdir(runs))
        root = runs / run_key / "sampler" / "uncapped_AG"
        return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(root) for f in fs}

    return run


def _chain(files, i):
    import io

    return np.load(io.BytesIO(files[f"predicted_samples/npy/{i}.npy"]))


def test_one_device_selected_in_process_writes_the_same_files(job):
    ref = job("auto", "~sampler.devices")
    assert len([f for f in ref if f.startswith("predicted_samples/npy/")]) == WALKERS * BATCHES + 1
    assert _chain(ref, 0).shape == (10, STEPS, 3) and np.isfinite(_chain(ref, 0)).all()
    for run_key, value in (("one", "1"), ("list0", "[0]")):
        got = job(run_key, f"sampler.devices={value}")
        assert sorted(got) == sorted(ref), value
        for f in ref:
            assert got[f] == ref[f], (value, f)
    # the rank side of a launch: jamun_sample as rank 0 of a one-rank job started by launch_ranks (RANK / WORLD_SIZE /
    # JAMUN_LOCAL_DEVICES set, a fresh child process) writes the same files too
    got = job("launched", launch_on=[0])
    assert sorted(got) == sorted(ref) and all(got[f] == ref[f] for f in ref)


def test_two_ranks_on_two_gpus(job):
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"{n} GPU visible: the two-rank launch needs two GPUs (the RCCL leg ran only as a one-rank group, tests/test_gpu_cli.py)")
    two = job("two", "sampler.devices=2", timeout=600)
    chains = sorted(int(f.split("/")[-1][:-4]) for f in two if f.startswith("predicted_samples/npy/") and not f.endswith("joined.npy"))
    assert chains == list(range(2 * WALKERS * BATCHES))
    seed42, seed43 = job("seed42", "seed=42"), job("seed43", "seed=43")
    # rank-major within each batch; rank r runs with seed 42 + r on its own GPU, and the walk is bit-reproducible across GPUs
    for b in range(BATCHES):
        for w in range(WALKERS):
            assert np.array_equal(_chain(two, 2 * WALKERS * b + w), _chain(seed42, WALKERS * b + w)), (b, w)
            assert np.array_equal(_chain(two, 2 * WALKERS * b + WALKERS + w), _chain(seed43, WALKERS * b + w)), (b, w)
    # sharded walkers: split over the ranks, not replicated; each shard draws its own initial noise, so only shapes are compared
    sh = job("sharded", "sampler.devices=2", "++sampler.shard_walkers=true", timeout=600)
    names = sorted(int(f.split("/")[-1][:-4]) for f in sh if f.startswith("predicted_samples/npy/") and not f.endswith("joined.npy"))
    assert names == list(range(WALKERS * BATCHES))
    for i in names:
        c = _chain(sh, i)
        assert c.shape == _chain(seed42, i).shape and np.isfinite(c).all(), i
