"""Does this checkpoint denoise?  ``scaled_rmsd`` of data frames at given noise levels — the number a training run logs as
``val/scaled_rmsd`` (``Denoiser.noise_and_compute_loss``, ``src/jamun/model/denoiser.py:219-297``) and ``VisualizeDenoiseMetrics`` reports
per dataset and sigma (``metrics/_visualize_denoise.py:100-122``, ``utils/scaled_rmsd.py``).

    python -m jamun_amd.denoise_eval --config-dir=configs experiment=sample_custom ++init_pdbs=[x.pdb] ++checkpoint_dir=ckpts \
                 ++sigma_list=[0.04,0.1] ++num_frames=64 ++align_noisy_input=true

composes the ``sample`` config of ``jamun_sample`` (`cmdline.compose`), reads ``init_datasets``, the checkpoint keys, ``seed`` and ``paths``
from it and ignores the sampler and batch-sampler nodes; ``sigma_list`` defaults to ``[${sigma}]``.  It runs inside the run directory, as
``jamun_sample`` does, and leaves ``denoise/<label>.npz`` and ``denoise/summary.json`` there.

Per frame: add sigma-noise to the frame, centre, Kabsch-align the noisy frame on the clean one, denoise, and report
scaled_rmsd = mean_i |xhat_i - x_i| / (sigma sqrt 3) with the raw and the weighted coordinate loss.  A checkpoint that denoises brings
scaled_rmsd well below 1, the value of returning the noisy frame.  Single process; multi-rank evaluation is out of scope.
"""

from __future__ import annotations

import json
import logging
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .data import WalkerBatch
from .model import compute_loss

log = logging.getLogger("jamun")

METRICS = ("scaled_rmsd", "raw_coordinate_loss", "coordinate_loss")


def metric_name(label: str, metric: str, sigma: float) -> str:
    """The reference's key (``_visualize_denoise.py:116``)."""
    return f"{label}/{metric}_per_dataset/sigma={sigma}"


def evaluate_denoiser(model, datasets: Sequence, sigma_list: Sequence[float], num_frames: Optional[int] = None, batch_size: int = 256,
                      align_noisy_input: bool = True, seed: Optional[int] = None, rng: str = "philox", output_dir: Optional[str] = "denoise") -> Dict[str, float]:
    """Noise, align, denoise and score the first ``num_frames`` frames (all if ``None``) of every dataset at every sigma of ``sigma_list``.

    Loop order: datasets in label order, each sigma, then batches of ``batch_size`` frames of that dataset; a short last batch is evaluated
    as its own batch, so a (dataset, sigma) pair uses at most two native samplers (one per batch width).  ``seed`` seeds torch's generators
    once, before the first draw; ``rng`` is `Denoiser.noise_and_denoise`'s.  Writes ``<output_dir>/<label>.npz`` (``sigma [S]``; ``scaled_rmsd``,
    ``raw_coordinate_loss``, ``coordinate_loss`` ``[S, F]`` float32, one column per frame) and ``<output_dir>/summary.json`` unless
    ``output_dir`` is None, and returns ``{"<label>/<metric>_per_dataset/sigma=<sigma>": mean over the frames}``, the means taken in float64
    on the host."""
    sigmas = [float(s) for s in sigma_list]
    if not sigmas:
        raise ValueError("sigma_list is empty")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be at least 1, got {batch_size}")
    if seed is not None:
        torch.manual_seed(int(seed))
    device = torch.device(model.device)
    results: Dict[str, float] = {}
    per_label: Dict[str, dict] = {}
    for dataset in sorted(datasets, key=lambda d: d.label()):
        label = dataset.label()
        if label in per_label:
            raise ValueError(f"two datasets carry the label {label!r}")
        F = len(dataset) if num_frames is None else min(int(num_frames), len(dataset))
        frames = [dataset[i] for i in range(F)]
        table = {m: np.zeros((len(sigmas), F), dtype=np.float32) for m in METRICS}
        # one batch (one topology, so one native sampler per sigma) per batch width; the frames' positions go in with `with_pos`
        widths: Dict[int, WalkerBatch] = {}
        for si, sigma in enumerate(sigmas):
            for lo in range(0, F, int(batch_size)):
                hi = min(lo + int(batch_size), F)
                if hi - lo not in widths:
                    widths[hi - lo] = WalkerBatch.from_molecules(frames[lo:hi], [label] * (hi - lo)).to(device)
                pos = torch.cat([f["pos"] for f in frames[lo:hi]], dim=0).to(device, torch.float32)
                x = widths[hi - lo].with_pos(pos)
                xhat, _ = model.noise_and_denoise(x, sigma, align_noisy_input, rng=rng)
                _, aux = compute_loss(x, xhat, sigma, model.mean_center, model.average_squared_distance)
                for m in METRICS:
                    table[m][si, lo:hi] = aux[m].detach().cpu().numpy()
            for m in METRICS:
                results[metric_name(label, m, sigma)] = float(table[m][si].astype(np.float64).mean()) if F else float("nan")
            log.info("%s sigma=%g: scaled_rmsd %.4f over %d frames", label, sigma, results[metric_name(label, "scaled_rmsd", sigma)], F)
        per_label[label] = dict(table, sigma=np.asarray(sigmas, dtype=np.float64))
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        for label, arrays in per_label.items():
            np.savez(os.path.join(output_dir, f"{label}.npz"), **arrays)
        summary = {"sigma_list": sigmas, "align_noisy_input": bool(align_noisy_input), "seed": seed, "rng": rng, "batch_size": int(batch_size),
                   "num_frames": {label: int(a["scaled_rmsd"].shape[1]) for label, a in per_label.items()}, "metrics": results}
        with open(os.path.join(output_dir, "summary.json"), "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)
    return results


def run(cfg: dict) -> Dict[str, float]:
    from . import config as C
    from .checkpoint import find_checkpoint

    # (the evaluation's own keys leave the config before it is resolved: the sample config does not declare them)
    own = {k: cfg.pop(k, d) for k, d in (("sigma_list", None), ("num_frames", None), ("align_noisy_input", True), ("batch_size", 256), ("rng", "philox"))}
    for k in ("sampler", "batch_sampler", "callbacks", "logger"):  # not read here, and their interpolations need not resolve
        cfg.pop(k, None)
    cfg = C.resolve(cfg, throw_on_missing=False)
    sigma_list = own["sigma_list"] if own["sigma_list"] is not None else [cfg["sigma"]]
    if not isinstance(sigma_list, (list, tuple)):
        sigma_list = [sigma_list]
    checkpoint_path = find_checkpoint(wandb_train_run_path=cfg.get("wandb_train_run_path"), checkpoint_dir=cfg.get("checkpoint_dir"),
                                      checkpoint_type=cfg.get("checkpoint_type"))
    cfg["model"]["checkpoint_path"] = checkpoint_path
    model = C.instantiate(cfg["model"])
    datasets = C.instantiate(cfg["init_datasets"])
    return evaluate_denoiser(model, datasets, sigma_list, num_frames=own["num_frames"], batch_size=int(own["batch_size"]),
                             align_noisy_input=bool(own["align_noisy_input"]), seed=cfg.get("seed"), rng=str(own["rng"]))


def main(argv: Optional[List[str]] = None) -> str:
    from . import cmdline
    from . import config as C

    argv = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO)
    cwd = os.getcwd()
    cfg = cmdline.compose(argv, cwd)
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
