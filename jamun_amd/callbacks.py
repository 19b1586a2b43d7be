"""Sampler callbacks: sample validation, metric dispatch and timing.  The trajectory writer, ``SaveTrajectoryCallback``,
lives in ``trajectory_writer.py`` and is re-exported here, where configurations and callers look for it."""

from __future__ import annotations

import json
import os
import time
from typing import List, Optional, Sequence

import torch

from .data import ATOM_TYPES
from .trajectory_writer import SaveTrajectoryCallback  # noqa: F401  (re-exported)


def validate_sample(sample, dataset) -> None:
    """``metrics/_utils.py:15-28``: the sample's label must be the dataset's and its atom types must be the topology's."""
    label = sample["dataset_label"] if "dataset_label" in sample else None
    if label != dataset.label():
        raise ValueError(f"Sample dataset label {label} does not match expected label {dataset.label()}.")
    mol = getattr(dataset, "molecule", None)
    if mol is None or "atom_type_index" not in sample:
        return
    name = lambda i: ATOM_TYPES[i] if 0 <= i < len(ATOM_TYPES) else "?"
    expected = [name(int(i)) for i in mol["atom_type_index"]]
    actual = [name(int(i)) for i in sample["atom_type_index"]]
    if expected != actual:
        raise ValueError(f"Atom types in init_graph ({actual}) do not match expected atom types in structure ({expected}).")


class TrajectoryMetricCallback:
    """Feeds per-walker samples to one metric object per dataset label (``callbacks/sampler/_utils.py:22-56``).

    ``metric_fn(dataset=...)`` builds the meter of a dataset; a meter offers ``update(sample)``, ``compute() -> dict`` and
    the hooks ``on_sample_start / on_after_sample_batch / on_sample_end`` (and optionally ``to(device)``), i.e. the
    reference's ``TrajectoryMetric`` protocol, so metric classes written against it plug in unchanged.  Datasets are
    de-duplicated by label and ordered by label."""

    def __init__(self, datasets: Sequence, metric_fn):
        unique = {}
        for d in datasets:
            unique.setdefault(d.label(), d)
        self.datasets = unique
        self.meters = {label: metric_fn(dataset=unique[label]) for label in sorted(unique)}

    def on_sample_start(self, sampler):
        for meter in self.meters.values():
            if hasattr(meter, "to"):
                meter.to(sampler.fabric.device)
            meter.on_sample_start()

    def on_after_sample_batch(self, sample: Sequence, sampler):
        for sample_graph in sample:
            validate_sample(sample_graph, self.datasets[sample_graph["dataset_label"]])  # TrajectoryMetric.update, metrics/_utils.py:64
            self.meters[sample_graph["dataset_label"]].update(sample_graph)
        for meter in self.meters.values():
            sampler.fabric.log_dict(meter.compute())
            meter.on_after_sample_batch()

    def on_sample_end(self, sampler):
        for meter in self.meters.values():
            meter.on_sample_end()


class RamachandranMetricsCallback(TrajectoryMetricCallback):
    """`TrajectoryMetricCallback` over `ramachandran.RamachandranMetrics` (the reference's ``RamachandranPlotMetricsCallback``,
    ``callbacks/sampler/ramachandran.yaml``, without its plots): per chain and for the joined trajectory the (phi, psi) histograms and
    the JS divergence from the true trajectory against the number of samples, under ``<output_dir>/<label>/ramachandran/``.  Keyword
    arguments go to the meter (``bins``, ``pairing``, ``reference``, ``output_dir``, ``sample_key``, ``device``)."""

    def __init__(self, datasets: Sequence, **kw):
        import functools

        from .ramachandran import RamachandranMetrics

        super().__init__(datasets, functools.partial(RamachandranMetrics, **kw))


class ChemicalValidityMetricsCallback(TrajectoryMetricCallback):
    """`TrajectoryMetricCallback` over `validity.ChemicalValidityMetrics` (the reference's ``ChemicalValidityMetricsCallback``,
    ``callbacks/sampler/chemical_validity.yaml``, without its wandb histograms): per checked frame the share of clashing non-bonded pairs
    and of bonds of a wrong length, under ``<output_dir>/<label>/chemical_validity/``.  Keyword arguments go to the meter
    (``volume_exclusion_tolerance``, ``bond_length_tolerance``, ``num_molecules_per_trajectory``, ``sample_key``, ``output_dir``,
    ``device``, ``vdw_radii``, ``covalent_radii``)."""

    def __init__(self, datasets: Sequence, **kw):
        import functools

        from .validity import ChemicalValidityMetrics

        super().__init__(datasets, functools.partial(ChemicalValidityMetrics, **kw))


class TICAMetricsCallback(TrajectoryMetricCallback):
    """`TrajectoryMetricCallback` over `tica.TICAMetrics` (the slow-mode part of the reference's ``analysis/run_analysis.py``: TICA fitted on
    the true trajectory, the samples projected on it): per chain and for the joined trajectory the first two components, the
    Jensen-Shannon distances of their histograms from the true trajectory's and the autocovariance of the first component, under
    ``<output_dir>/<label>/tica/``.  Keyword arguments go to the meter (``lag``, ``max_acf_lag``, ``features``, ``bins_1d``, ``bins_2d``,
    ``var_cutoff``, ``epsilon``, ``kinetic_map``, ``reference``, ``device``, ``output_dir``, ``sample_key``)."""

    def __init__(self, datasets: Sequence, **kw):
        import functools

        from .tica import TICAMetrics

        super().__init__(datasets, functools.partial(TICAMetrics, **kw))


class MSMMetricsCallback(TrajectoryMetricCallback):
    """`TrajectoryMetricCallback` over `msm.MSMMetrics` (the Markov-state-model part of the reference's ``analysis/run_analysis.py``:
    ``compute_MSM_stats``): k-means, a Markov state model and its metastable states fitted on the TICA projection of the true trajectory;
    per chain and for the joined trajectory the occupancies of the metastable states, their Jensen-Shannon distance from the true ones
    (also against the number of samples) and the transition counts and matrix at ``traj_lag``, under ``<output_dir>/<label>/msm/``.
    Keyword arguments go to the meter (``k``, ``max_iter``, ``seed``, ``msm_lag``, ``n_metastable``, ``traj_lag``, ``n_steps``, ``lag``,
    ``features``, ``var_cutoff``, ``epsilon``, ``kinetic_map``, ``reference``, ``device``, ``output_dir``, ``sample_key``)."""

    def __init__(self, datasets: Sequence, **kw):
        import functools

        from .msm import MSMMetrics

        super().__init__(datasets, functools.partial(MSMMetrics, **kw))


class SlicedWassersteinMetricsCallback(TrajectoryMetricCallback):
    """`TrajectoryMetricCallback` over `swd.SlicedWassersteinMetrics` (the second curve of the reference's ``RamachandranPlotMetrics``:
    ``compute_sliced_Wasserstein_distance_vs_num_samples``, without the ``ot`` package): per chain and for the joined trajectory the
    sliced Wasserstein distance of the (cos, sin) descriptors of phi and psi from the true trajectory's against the number of samples,
    under ``<output_dir>/<label>/sliced_wasserstein/``.  Keyword arguments go to the meter (``n_projections``, ``seed``, ``pairing``,
    ``reference``, ``output_dir``, ``sample_key``, ``device``)."""

    def __init__(self, datasets: Sequence, **kw):
        import functools

        from .swd import SlicedWassersteinMetrics

        super().__init__(datasets, functools.partial(SlicedWassersteinMetrics, **kw))


class MeasureSamplingTimeCallback:
    """Wall time per batch and per sampled conformation (one saved (walker, frame) pair — the reference's unit,
    ``callbacks/sampler/_measure_sampling_time.py:57,71``).  Writes ``sampler/timing.json`` on rank 0."""

    def __init__(self, output_dir: str = "sampler", **_):
        self.output_dir = output_dir
        self.t0: Optional[float] = None
        self.batches: List[dict] = []

    def on_sample_start(self, sampler):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def on_after_sample_batch(self, sample: Sequence[dict], sampler):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        n_conf = sum(int(s["xhat_traj"].shape[1]) for s in sample if "xhat_traj" in s)
        self.batches.append({"batch": int(sampler.global_step), "seconds": t1 - self.t0, "conformations": n_conf})
        self.t0 = t1

    def on_sample_end(self, sampler):
        if not sampler.is_global_zero:
            return
        os.makedirs(self.output_dir, exist_ok=True)
        tot_s = sum(b["seconds"] for b in self.batches)
        tot_c = sum(b["conformations"] for b in self.batches)
        with open(os.path.join(self.output_dir, "timing.json"), "w") as f:
            json.dump({"batches": self.batches, "rank0_conformations_per_second": tot_c / tot_s if tot_s > 0 else None,
                       "ms_per_sample": 1e3 * tot_s / tot_c if tot_c else None, "world_size": sampler.world_size}, f, indent=1)
