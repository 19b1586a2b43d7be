"""``jamun_sample`` — entry point of the sampling path (mirror of ``/root/reference/src/jamun/cmdline/sample.py:41-138``).

    jamun_sample --config-dir=configs experiment=sample_custom ++init_pdbs=[x.pdb] ++checkpoint_dir=ckpts \
                 num_sampling_steps_per_batch=50 repeat_init_samples=4

Accepts the reference's command-line form (``--config-dir``, ``experiment=...``, ``key=value``, ``++key=value``) and its
config keys.  Differences, all explicit: no wandb (``wandb_train_run_path`` must be null; use ``checkpoint_dir``),
``finetune_on_init`` must be null/false (training is out of scope), ``sampler.accelerator=cpu`` /
``trainer.accelerator=cpu`` is rejected (there is no CPU path).

``sampler.devices`` (``jamun_amd.dist.resolve_devices``) asking for more than one GPU starts one rank per GPU, as the reference's
``fabric.launch()`` does: the same command line runs in each rank with one shared ``run_key`` (`launch_plan`).
"""

from __future__ import annotations

import json
import logging
import os
import sys
from typing import List, Optional, Sequence, Tuple

import torch

from . import config as C
from . import dist
from .checkpoint import find_checkpoint
from .data import WalkerBatch

log = logging.getLogger("jamun")


def get_initial_graphs(datasets: Sequence, num_init_samples_per_dataset: int, repeat: int = 1) -> WalkerBatch:
    """``cmdline/sample.py:27-38``: per dataset ``randperm(len)[:k]`` frames, each repeated ``repeat`` times (consecutive)."""
    mols, labels = [], []
    for dataset in datasets:
        random_indices = torch.randperm(len(dataset))[:num_init_samples_per_dataset].tolist()
        # The reference draws this before any seed is set (sample.py:33 vs :86-88), so ranks may pick different frames.  Here
        # rank 0's draw is used on every rank: with sharded walkers the shards must partition ONE initial batch.
        random_indices = dist.broadcast_object(random_indices, src=0)
        for index in random_indices:
            g = dataset[int(index)]
            for _ in range(repeat):
                mols.append(g)
                labels.append(dataset.label())
    return WalkerBatch.from_molecules(mols, labels)


def run(cfg: dict):
    cfg = C.resolve(cfg, throw_on_missing=True)
    if cfg.get("finetune_on_init"):
        raise NotImplementedError("finetune_on_init is a training feature and is out of scope; pass finetune_on_init=null")
    if isinstance(cfg.get("trainer"), dict) and "accelerator" in cfg["trainer"]:
        cfg["sampler"]["accelerator"] = cfg["trainer"]["accelerator"]  # BASELINE.json's spelling of sampler.accelerator
    checkpoint_path = find_checkpoint(
        wandb_train_run_path=cfg.get("wandb_train_run_path"),
        checkpoint_dir=cfg.get("checkpoint_dir"),
        checkpoint_type=cfg.get("checkpoint_type"),
    )
    cfg["model"]["checkpoint_path"] = checkpoint_path
    model = C.instantiate(cfg["model"])
    init_datasets = C.instantiate(cfg["init_datasets"])
    callbacks = []
    for _, node in (cfg.get("callbacks") or {}).items():
        if isinstance(node, dict) and "_target_" in node:
            # ${init_datasets} resolved to the config node; hand the callback the instantiated datasets instead
            extra = {"datasets": init_datasets} if "datasets" in node else {}
            callbacks.append(C.instantiate({k: v for k, v in node.items() if k != "datasets"}, **extra))
    init_graphs = get_initial_graphs(init_datasets, cfg["num_init_samples_per_dataset"], cfg.get("repeat_init_samples", 1))
    sampler = C.instantiate(cfg["sampler"], callbacks=callbacks, loggers=None)
    batch_sampler = C.instantiate(cfg["batch_sampler"])
    if seed := cfg.get("seed"):
        torch.manual_seed(seed + sampler.fabric.global_rank)  # ranks generate different chains (sample.py:86-88)
    log.info("sampling %d walkers (%d atoms) on %s", init_graphs.num_graphs, init_graphs.num_nodes, sampler.device)
    sampler.sample(model=model, batch_sampler=batch_sampler, init_graphs=init_graphs, num_batches=cfg["num_batches"],
                   continue_chain=cfg["continue_chain"])
    return sampler


def compose(argv: List[str], cwd: Optional[str] = None) -> dict:
    cwd = cwd or os.getcwd()
    dirs, overrides = [], []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("--config-dir="):
            dirs.append(a.split("=", 1)[1])
        elif a in ("--config-dir", "-cd"):
            dirs.append(argv[i + 1])
            i += 1
        elif a.startswith("--"):
            raise SystemExit(f"unsupported flag {a}")
        else:
            overrides.append(a)
        i += 1
    composer = C.Composer([os.path.abspath(os.path.join(cwd, d)) for d in dirs] + [C.BUILTIN_DIR])
    cfg = composer.compose("sample", overrides)
    # make user paths absolute before changing into the run directory (hydra job.chdir = true)
    if isinstance(cfg.get("init_pdbs"), list):
        cfg["init_pdbs"] = [p if os.path.isabs(p) or "${" in str(p) else os.path.join(cwd, p) for p in cfg["init_pdbs"]]
    ck = cfg.get("checkpoint_dir")
    if isinstance(ck, str) and ck != C.MISSING and not os.path.isabs(ck) and "${" not in ck:
        cfg["checkpoint_dir"] = os.path.join(cwd, ck)
    return cfg


def launch_plan(cfg: dict, argv: List[str], environ: Optional[dict] = None) -> Optional[Tuple[List[int], List[str]]]:
    """``(devices, rank command)`` when ``jamun_sample`` must start one rank per device of ``sampler.devices``; ``None`` when this
    process samples itself: ``auto``, one device, or already a rank of a launched job (``WORLD_SIZE`` set).  ``run_key`` (default
    ``${now:...}``) is resolved once here and passed to every rank, so that all ranks write into one run directory."""
    environ = os.environ if environ is None else environ
    if "WORLD_SIZE" in environ:
        return None
    r = C.resolve(cfg, throw_on_missing=False)
    smp = r.get("sampler") or {}
    devices = dist.resolve_devices(smp.get("devices", "auto"), smp.get("num_nodes", 1))
    if devices is None or len(devices) < 2:
        return None
    return devices, [sys.executable, "-m", "jamun_amd.cmdline", *argv, "++run_key=" + json.dumps(r["run_key"])]


def main(argv: Optional[List[str]] = None):
    argv = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO)
    cwd = os.getcwd()
    cfg = compose(argv, cwd)
    plan = launch_plan(cfg, argv)
    if plan is not None:  # this process makes no GPU call: each rank opens its own
        devices, cmd = plan
        log.info("sampler.devices: starting %d ranks on GPUs %s", len(devices), ",".join(map(str, devices)))
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the ranks import this copy of the package
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p))
        sys.exit(dist.launch_ranks(cmd, devices, env=env))
    dist.init_process_group()
    head = C.resolve({k: cfg[k] for k in ("paths", "task_name", "run_group", "run_key")})
    run_dir = head["paths"]["run_path"]
    run_dir = run_dir if os.path.isabs(run_dir) else os.path.join(cwd, run_dir)
    os.makedirs(run_dir, exist_ok=True)
    os.chdir(run_dir)
    try:
        run(cfg)
    finally:
        os.chdir(cwd)
    return run_dir


if __name__ == "__main__":
    main()
