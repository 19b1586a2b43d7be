"""The trajectory writer of a sampling run.

``SaveTrajectoryCallback`` writes the file set of the reference's ``SaveTrajectory`` metric
(``src/jamun/metrics/_save_trajectory.py:17-30,53-56,78-97``, ``metrics/_utils.py:84-113``) under ``sampler/<label>/``:

    topology.pdb                                   first frame of the dataset            (on_sample_start)
    predicted_samples/npy/<i>.npy   [n, T, 3] nm   one per chain                         (every batch)
    predicted_samples/pdb/<i>.pdb, dcd/<i>.dcd     the same chain as PDB models / CHARMM DCD (Angstrom)
    predicted_samples/{npy,pdb,dcd}/joined.*       all chains so far, frames concatenated: [n, chains*T, 3]

``analysis/load_trajectory.py:88-107`` needs ``dcd/joined.dcd`` plus ``topology.pdb`` (or ``pdb/0.pdb``).  Samples are
dispatched by ``dataset_label`` (``callbacks/sampler/_utils.py:42-52``) and validated against the dataset
(``metrics/_utils.py:15-28``).  With several ranks the per-rank blocks are gathered to rank 0 once per batch and label
(``jamun_amd.dist.gather_ragged``) — what torchmetrics' ``dist_reduce_fx="cat"`` does in the reference.

A batch of one label is written by `_write_batch` on the writer thread: on the host path `_write_chain` per chain and `_write_joined`;
on the device path `_write_batch_device`, which makes a `_BatchPlan` (what the encoder can take, in chunks of how many frames), runs
the jobs of `_chain_jobs` chain by chain and lets the host formatter write what `_host_fallbacks` names.  What the writer remembers
between batches is one `_LabelState` per label.
"""

from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass, field
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, dist
from .features import internal_coords_host, torsion_indices
from .pdb import append_dcd_frames, append_pdb_models, save_dcd, save_pdb
from .superpose import superpose_host
from .traj_encode import DeviceTrajectoryEncoder


@dataclass
class _LabelState:
    """What the writer keeps per dataset label."""
    dataset: object
    mol: Optional[dict]  # the dataset's molecule if it carries atom names (.pdb text needs them), else None
    chains: List[np.ndarray] = field(default_factory=list)  # every chain so far, [n, T, 3] each
    num_chains_seen: int = 0
    joined_frames: int = 0  # models / frames in joined.pdb / joined.dcd
    ref: Optional[np.ndarray] = None  # superpose: the reference structure [n, 3] (float32, nm) ...
    rmsd: List[np.ndarray] = field(default_factory=list)  # ... and per chain the RMSD of its frames, [T] each
    tor_index: Optional[np.ndarray] = None  # torsions: the index table int32 [F, 4] ...
    tor_labels: Optional[List[str]] = None  # ... the labels of its rows ...
    tor: List[np.ndarray] = field(default_factory=list)  # ... and per chain the torsions of its frames, [T, F] each
    dev: Dict[str, torch.Tensor] = field(default_factory=dict)  # the device copies of ``ref`` and ``tor_index`` (`_device_copy`)


@dataclass
class _BatchPlan:
    """How the chains of one label and batch go through the encoder.  A chunk size is in frames; 0: the encoder does not do that job
    (switched off, no template, or one frame larger than the staging memory) and the host does where the file is wanted."""
    tmpl: Optional[Tuple[torch.Tensor, torch.Tensor]]  # `DeviceTrajectoryEncoder.template` of the molecule, None: no .pdb text from the device
    pdb_chunk: int
    dcd_chunk: int
    align_chunk: int = 0
    tor_chunk: int = 0
    ref_dev: Optional[torch.Tensor] = None
    tor_index_dev: Optional[torch.Tensor] = None


def _device_copy(st: _LabelState, name: str, enc: DeviceTrajectoryEncoder) -> torch.Tensor:
    """The host table ``st.<name>`` on the encoder's device: uploaded on the encoder's stream once, then kept."""
    if name not in st.dev or st.dev[name].device != enc.device:
        with torch.cuda.device(enc.device), torch.cuda.stream(enc.stream):
            st.dev[name] = torch.from_numpy(getattr(st, name)).to(enc.device)
    return st.dev[name]


def _chunks(lo: int, hi: int, step: int) -> List[Tuple[int, int]]:
    """[lo, hi) in pieces (t0, t1) of ``step`` frames; none for step 0."""
    return [(t, min(hi, t + step)) for t in range(lo, hi, step)] if step > 0 else []


def _keep(dst: np.ndarray, a: int, b: int, data) -> None:
    """Sink: a chunk's float32 bytes are rows a:b of ``dst``."""
    dst[a:b] = np.frombuffer(data, dtype=np.float32).reshape(dst[a:b].shape)


def _append_dcd(paths: Sequence[str], n: int, k: int, data) -> None:
    """Sink: ``k`` encoded frames of ``n`` atoms go to the end of each file."""
    for path in paths:
        append_dcd_frames(path, n, data, k)


def _chain_jobs(enc, plan: _BatchPlan, frames: torch.Tensor, own: dict, joined: dict, joined_at: int, rmsd, tor) -> list:
    """The (encode, sink) jobs of one chain for `DeviceTrajectoryEncoder.run`, ``frames`` its [T, n, 3] device view.  Per span of frames
    (the whole chain, or with ``superpose`` what the aligned scratch holds): superpose it, RMSD into ``rmsd``; its PDB chunks, to the
    chain's own file and, numbered on from ``joined_at``, to the joined one; its DCD chunks, to both files.  Then the torsions of the RAW
    chain, chunk by chunk into ``tor``.  ``own`` / ``joined``: the paths by extension."""
    (T, n), jobs = frames.shape[:2], []
    for s0, s1 in _chunks(0, T, plan.align_chunk) or [(0, T)]:
        view = frames[s0:s1]
        if plan.align_chunk > 0:  # superposed into the encoder's scratch; the RMSD leaves as the job's bytes
            view = enc.align_view(n, s1 - s0)
            jobs.append((enc.superpose(frames[s0:s1], plan.ref_dev, view), partial(_keep, rmsd, s0, s1)))
        for t0, t1 in _chunks(s0, s1, plan.pdb_chunk):
            jobs.append((enc.encode_pdb(view[t0 - s0 : t1 - s0], t0, *plan.tmpl), partial(append_pdb_models, own["pdb"])))
            jobs.append((enc.encode_pdb(view[t0 - s0 : t1 - s0], joined_at + t0, *plan.tmpl), partial(append_pdb_models, joined["pdb"])))
        for t0, t1 in _chunks(s0, s1, plan.dcd_chunk):
            jobs.append((enc.encode_dcd(view[t0 - s0 : t1 - s0]), partial(_append_dcd, (own["dcd"], joined["dcd"]), n, t1 - t0)))
    for t0, t1 in _chunks(0, T, plan.tor_chunk):
        jobs.append((enc.features(frames[t0:t1], plan.tor_index_dev), partial(_keep, tor, t0, t1)))
    return jobs


def _unlink(paths) -> None:
    for path in paths:
        if os.path.exists(path):
            os.unlink(path)


class SaveTrajectoryCallback:
    """The file set of the reference's ``SaveTrajectory`` metric (``metrics/_save_trajectory.py:17-97``) under
    ``<output_dir>/<label>/``: ``topology.pdb``; ``predicted_samples/{npy,pdb,dcd}/<i>.*`` per chain and ``joined.*``; with
    ``save_true_trajectory`` also ``true_samples/{pdb,dcd}/0.*`` = the dataset's own frames (``:22-26,58-62``).

    One deliberate deviation: the reference numbers the ``.pdb`` / ``.dcd`` files of a batch from the running chain count but
    restarts the ``.npy`` numbering at 0 in every batch (``enumerate(samples_np)`` at ``:81`` against ``start=self.num_chains_seen``
    at ``:89``), so its ``<i>.npy`` files of batch b overwrite those of batch b-1 and only ``joined.npy`` keeps everything.  Here all
    three use the running index; ``npy_index_restarts_per_batch=True`` reproduces the reference's files exactly.

    ``encode`` selects who turns frames into ``.pdb`` text and ``.dcd`` records.  ``"host"``: `pdb.save_pdb` / `pdb.save_dcd` on the
    host copy of the batch, every file rewritten whole (``joined.*`` from every chain seen so far).  ``"device"``: the stacked
    device block of the batch is kept until the writer thread has encoded it on the GPU (`traj_encode.DeviceTrajectoryEncoder`,
    chunks of frames through fixed staging memory on one side stream) and ``joined.pdb`` / ``joined.dcd`` are EXTENDED by the new
    chains' frames; the files are byte for byte those of ``"host"``.  ``"auto"`` (default) takes the device path when the sample
    tensors are on a GPU, the native library loads and no process group is initialised (the multi-rank gather delivers host
    blocks: it keeps the host path), else the host path.  ``.npy`` files are written from the host copy either way.

    ``superpose=True`` writes every ``.pdb`` / ``.dcd`` frame (per chain and ``joined``) superposed on the label's reference structure,
    its dataset molecule's ``pos`` — the init structure, what the reference's consumers align on (``dataset.trajectory[0]``,
    ``metrics/_visualize_samples.py:26-28``): the best proper rotation and translation per frame (`superpose.superpose_host`; on the
    device path ``jamun_superpose.hip`` on the encoder's side stream, in front of the encoders).  The ``.npy`` files stay the raw
    sampler output (the lossless record), and ``predicted_samples/rmsd/<i>.npy`` (float32 ``[T]``, nm: each frame's RMSD to the reference
    after the fit) and ``rmsd/joined.npy`` (their concatenation) appear.  Off (default) nothing changes.

    ``torsions`` adds the torsion angles of every frame: ``True`` or ``"backbone"`` phi, psi and omega, ``"all"`` the side-chain chi1..chi4
    besides (`features.torsion_indices`: by atom names, mdtraj's rule; the dataset's molecule must carry names).  Per label
    ``<label>/torsion_labels.json`` (the labels and atom indices of the F columns) and ``predicted_samples/torsions/<i>.npy`` (float32
    ``[T, F]``, radians, dihedrals in (-pi, pi]) per chain, ``torsions/joined.npy`` their concatenation over all chains so far on axis 0.
    The values come from the raw sampler output (internal coordinates do not change under superposition: the files are the same with
    ``superpose`` on and off): `features.internal_coords_host` on the host path, ``jamun_intcoord.hip`` on the encoder's side stream on the
    device path.  Off (``False``, default) nothing changes."""

    def __init__(self, datasets: Sequence, sample_key: str = "xhat_traj", output_dir: str = "sampler", write_pdb: bool = True,
                 write_dcd: bool = True, save_true_trajectory: bool = False, npy_index_restarts_per_batch: bool = False,
                 async_write: bool = True, encode: str = "auto", superpose: bool = False, torsions=False, **_):
        if encode not in ("auto", "host", "device"):
            raise ValueError(f"encode must be 'auto', 'host' or 'device', got {encode!r}")
        if torsions is None or torsions is False:
            self.torsions = None
        elif torsions is True or torsions == "backbone":
            self.torsions = "backbone"
        elif torsions == "all":
            self.torsions = "all"
        else:
            raise ValueError(f"torsions must be False, True, 'backbone' or 'all', got {torsions!r}")
        self.encode = encode
        self.sample_key = sample_key
        self.output_dir = output_dir
        self.write_pdb = write_pdb
        self.write_dcd = write_dcd
        self.save_true_trajectory = save_true_trajectory
        self.npy_index_restarts_per_batch = npy_index_restarts_per_batch
        self.superpose = bool(superpose)
        first = {d.label(): d for d in reversed(list(datasets))}  # (of two datasets with one label the first counts)
        self._states: Dict[str, _LabelState] = {label: self._label_state(first[label], torsions) for label in sorted(first)}
        self.labels = list(self._states)  # (sorted: the order of the gathers and of the writes)
        self.chains = {label: st.chains for label, st in self._states.items()}  # per label the list its state holds: [n, T, 3] each
        # Files are written on ONE side thread, in submission order, while the next batch walks on the GPU (the walk is a single native call
        # that releases the GIL; numpy's file writes release it too): a 20 000-step batch of 256 dipeptides is 1 GB per key, and its files
        # take as long to write as the GPU needs for the walk.  on_sample_end (and flush) wait for the writer; wait_s is that time.
        self.async_write = bool(async_write)
        self._pool = None
        self._pending: list = []
        self.wait_s = 0.0
        self._stager = dist.HostStager()  # one pinned + one device staging buffer for the whole run (dist.gather_ragged_to_host)
        self.gather_timings: Dict[str, float] = {}  # gather_s / gather_bytes accumulated over batches and labels (bench.py: e2e_sharded)
        self._encoder = None  # traj_encode.DeviceTrajectoryEncoder, created with the first device-encoded batch
        self._dev_blocks: dict = {}  # (label, first chain index) -> (device block [chains, n, T, 3], event recorded behind its producer)

    def _label_state(self, dataset, torsions) -> _LabelState:
        label, mol = dataset.label(), getattr(dataset, "molecule", None)
        st = _LabelState(dataset=dataset, mol=mol if (mol is not None and "atom_names" in mol) else None)
        if self.superpose:
            if mol is None or mol.get("pos") is None:
                raise ValueError(f"SaveTrajectoryCallback(superpose=True): the dataset of label {label!r} has no molecule, so no reference "
                                 "structure to superpose on")
            pos = mol["pos"]
            st.ref = np.ascontiguousarray(pos.detach().cpu().numpy() if torch.is_tensor(pos) else pos, dtype=np.float32)
        if self.torsions is not None:
            if mol is None:
                raise ValueError(f"SaveTrajectoryCallback(torsions={torsions!r}): the dataset of label {label!r} has no molecule to find torsions in")
            st.tor_index, st.tor_labels = torsion_indices(mol, backbone=True, sidechain=self.torsions == "all")
        return st

    @property
    def num_chains_seen(self) -> Dict[str, int]:
        return {label: st.num_chains_seen for label, st in self._states.items()}

    def _dir(self, label: str, ext: str) -> str:
        d = os.path.join(self.output_dir, label, "predicted_samples", ext)
        os.makedirs(d, exist_ok=True)
        return d

    def filename_pred(self, label: str, trajectory_index, extension: str) -> str:
        if extension not in ("npy", "pdb", "dcd"):
            raise ValueError(f"Invalid extension: {extension}")
        return os.path.join(self._dir(label, extension), f"{trajectory_index}.{extension}")

    def filename_rmsd(self, label: str, trajectory_index) -> str:
        """``predicted_samples/rmsd/<i>.npy`` (superpose=True): float32 [T], the frames' RMSD in nm to the reference structure."""
        return os.path.join(self._dir(label, "rmsd"), f"{trajectory_index}.npy")

    def filename_torsions(self, label: str, trajectory_index) -> str:
        """``predicted_samples/torsions/<i>.npy`` (torsions on): float32 [T, F], the frames' torsion angles in radians."""
        return os.path.join(self._dir(label, "torsions"), f"{trajectory_index}.npy")

    def on_sample_start(self, sampler):
        if not sampler.is_global_zero:
            return
        for label, st in self._states.items():
            root = os.path.join(self.output_dir, label)
            for ext in ("npy", "pdb", "dcd"):
                self._dir(label, ext)
            if self.torsions is not None:
                with open(os.path.join(root, "torsion_labels.json"), "w") as f:
                    json.dump({"labels": st.tor_labels, "atom_indices": st.tor_index.tolist(), "unit": "rad"}, f, indent=1)
            if st.mol is not None and self.write_pdb:  # topology from the dataset's first frame (_save_trajectory.py:53-56)
                save_pdb(os.path.join(root, "topology.pdb"), st.mol, st.mol["pos"][None])
            if not self.save_true_trajectory:
                continue
            # the dataset's own frames as true_samples/{pdb,dcd}/0.* (_save_trajectory.py:22-26,58-62): its xyz, else a named molecule's structure
            frames = getattr(st.dataset, "xyz", None)
            if frames is None and st.mol is not None:
                frames = st.mol["pos"][None]
            if frames is None:
                continue
            frames = frames.detach().cpu().numpy()
            for ext in ("pdb", "dcd"):
                os.makedirs(os.path.join(root, "true_samples", ext), exist_ok=True)
            if st.mol is not None:
                save_pdb(os.path.join(root, "true_samples", "pdb", "0.pdb"), st.mol, frames)
            save_dcd(os.path.join(root, "true_samples", "dcd", "0.dcd"), frames)

    def _host_frames(self, st: _LabelState, arr: np.ndarray):
        """arr [n, T, 3] -> (its frames [T, n, 3] as the .pdb / .dcd files show them: superposed on the label's reference structure with
        ``superpose``; their RMSD to it [T], else None) on the host."""
        frames = np.transpose(arr, (1, 0, 2))  # "atoms frames coords -> frames atoms coords" (utils/mdtraj.py:17-21)
        return superpose_host(frames, st.ref) if self.superpose else (frames, None)

    def _torsions_host(self, st: _LabelState, arr: np.ndarray) -> Optional[np.ndarray]:
        """arr [n, T, 3] (raw) -> the torsions of its frames float32 [T, F] on the host (None with ``torsions`` off)."""
        return internal_coords_host(np.transpose(arr, (1, 0, 2)), st.tor_index).astype(np.float32) if self.torsions is not None else None

    def _save_host(self, st: _LabelState, label: str, index, frames: np.ndarray, pdb: bool = True, dcd: bool = True) -> None:
        """``<index>.pdb`` / ``<index>.dcd`` of ``frames`` [T, n, 3] by the host formatter, each where it is switched on (and asked for)."""
        if pdb and self.write_pdb and st.mol is not None:
            save_pdb(self.filename_pred(label, index, "pdb"), st.mol, frames)
        if dcd and self.write_dcd:
            save_dcd(self.filename_pred(label, index, "dcd"), frames)

    def _save_chain_side_files(self, st: _LabelState, label: str, index: int, tor, rmsd) -> None:
        """``torsions/<index>.npy`` and ``rmsd/<index>.npy`` of a chain; the arrays are kept, the joined files are their concatenation."""
        if self.torsions is not None:
            st.tor.append(tor)
            np.save(self.filename_torsions(label, index), tor)
        if self.superpose:
            st.rmsd.append(rmsd)
            np.save(self.filename_rmsd(label, index), rmsd)

    def _save_joined_side_files(self, st: _LabelState, label: str, rmsd=None) -> None:
        """``torsions/joined.npy`` and ``rmsd/joined.npy`` from the chains' arrays (``rmsd``: that of joined frames superposed again)."""
        if self.torsions is not None:
            np.save(self.filename_torsions(label, "joined"), np.concatenate(st.tor))
        if self.superpose:
            np.save(self.filename_rmsd(label, "joined"), np.concatenate(st.rmsd) if rmsd is None else rmsd)

    def _write_chain(self, label: str, index: int, arr: np.ndarray) -> None:
        """arr [n, T, 3] nm -> <index>.pdb / .dcd and the chain's side files on the host path"""
        st = self._states[label]
        frames, rmsd = self._host_frames(st, arr)
        self._save_chain_side_files(st, label, index, self._torsions_host(st, arr), rmsd)
        self._save_host(st, label, index, frames)

    def _write_joined(self, label: str, arr: np.ndarray) -> None:
        """arr [n, chains * T, 3], every chain so far -> joined.pdb / .dcd and side files on the host path: rewritten whole and superposed
        again (the reference's behaviour, _save_trajectory.py:84-97)"""
        st = self._states[label]
        frames, rmsd = self._host_frames(st, arr)
        self._save_joined_side_files(st, label, rmsd)
        self._save_host(st, label, "joined", frames)

    def _finished_writer_error(self) -> Optional[BaseException]:
        """A writer failure (disk full, permission, bad shape) must stop the run at the NEXT batch, not after the last one.  It is
        returned, not raised: only rank 0 writes, and the other ranks learn of it in the gather (raising here would leave them waiting
        in the gather's collectives)."""
        still, error = [], None
        for fut in self._pending:
            if not fut.done():
                still.append(fut)
            elif error is None:
                error = fut.exception()
        self._pending = still
        return error

    def _labels_encoded_on_device(self, sample: Sequence[dict]) -> set:
        """The one decision for a batch: the labels whose chains the GPU encodes (``encode``; all sample tensors on a GPU, no process
        group, the library; something to encode; the label's chains float32 with at least one frame).  Every other label takes the host path."""
        mine = [s for s in sample if self.sample_key in s]
        if self.encode == "host" or not mine:  # (or nothing to write)
            return set()
        on_gpu = all(torch.is_tensor(s[self.sample_key]) and s[self.sample_key].is_cuda for s in mine)
        grouped = torch.distributed.is_available() and torch.distributed.is_initialized()
        if self.encode == "device":
            if not on_gpu:
                raise RuntimeError("SaveTrajectoryCallback(encode='device') needs the sample tensors on a GPU; use encode='host' (or 'auto') for CPU tensors")
            if grouped:
                raise RuntimeError("SaveTrajectoryCallback(encode='device') does not run under a process group: the trajectory gather delivers host blocks")
            _lib.load()
        elif not on_gpu or grouped or not _lib.available():
            return set()
        if not (self.write_dcd or self.write_pdb or self.torsions is not None):
            return set()
        encodable = lambda t: t.dtype == torch.float32 and t.ndim == 3 and t.shape[1] > 0
        return {label for label in {s.get("dataset_label") for s in mine}
                if all(encodable(s[self.sample_key]) for s in mine if s.get("dataset_label") == label)}

    def on_after_sample_batch(self, sample: Sequence[dict], sampler):
        from .callbacks import validate_sample  # (callbacks.py imports this module)

        error = self._finished_writer_error()
        on_device = self._labels_encoded_on_device(sample)
        for s in sample:
            if s.get("dataset_label") not in self._states:
                raise KeyError(f"sample dataset label {s.get('dataset_label')!r} has no dataset")
        for label, st in self._states.items():
            mine = [s for s in sample if s.get("dataset_label") == label]
            for s in mine:
                validate_sample(s, st.dataset)
                if s[self.sample_key].ndim != 3:
                    raise ValueError(f"Invalid sample shape: {tuple(s[self.sample_key].shape)}, expected (num_atoms, num_frames, 3).")
            # a rank without walkers of this label contributes nothing; gather_ragged agrees on the trailing shape first
            block = torch.stack([s[self.sample_key] for s in mine]).contiguous() if mine else None  # [chains_local, n, T, 3]
            # one block at a time through ONE reusable device receive buffer and ONE reusable pinned staging buffer; what the writer
            # thread (and the label's chains) keep are pageable copies
            blocks = dist.gather_ragged_to_host(block, dst=0, device=sampler.device, stager=self._stager, timings=self.gather_timings,
                                                error=error)
            if blocks is None:
                continue
            start = st.num_chains_seen
            st.num_chains_seen = start + sum(int(b.shape[0]) for b in blocks)
            if label in on_device:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(block.device))
                self._dev_blocks[(label, start)] = (block, ready)  # kept alive until the writer thread has encoded it
            self._submit(self._write_batch, label, blocks, start)
        if error is not None:  # (no label, so no gather to carry it)
            raise error

    def _write_batch(self, label: str, blocks: List[np.ndarray], start: int) -> None:
        st = self._states[label]
        dev = self._dev_blocks.pop((label, start), None)
        new = [c for b in blocks for c in b]
        st.chains.extend(new)
        for i, arr in enumerate(new, start=start):  # the .npy files: the raw sampler output, from the host copy on either path
            np.save(self.filename_pred(label, (i - start) if self.npy_index_restarts_per_batch else i, "npy"), arr)
        if not st.chains:
            return
        joined = np.concatenate(st.chains, axis=1)  # "b n t c -> n (b t) c" (axis 1: joined.npy cannot be appended)
        np.save(self.filename_pred(label, "joined", "npy"), joined)
        if dev is not None:
            self._write_batch_device(label, new, joined, start, *dev)
        else:
            for i, arr in enumerate(new, start=start):
                self._write_chain(label, i, arr)
            self._write_joined(label, joined)
        st.joined_frames = int(joined.shape[1])

    def _plan(self, st: _LabelState, label: str, enc, n: int) -> _BatchPlan:
        """What the encoder does for this label's chains of ``n`` atoms and in chunks of how many frames; uploads the label's tables."""
        mol = st.mol if self.write_pdb else None
        tmpl = None
        if mol is not None and len(mol["atom_names"]) == n and n + 1 <= 99999:
            try:
                tmpl = enc.template(mol)
            except UnicodeEncodeError:
                tmpl = None
        plan = _BatchPlan(tmpl=tmpl, pdb_chunk=enc.pdb_frames_per_chunk(int(tmpl[0].numel())) if tmpl is not None else 0,
                          dcd_chunk=enc.dcd_frames_per_chunk(n) if self.write_dcd else 0)
        if self.superpose:
            if st.ref.shape[0] != n:
                raise ValueError(f"superpose: the reference structure of {label!r} has {st.ref.shape[0]} atoms, the samples have {n}")
            plan.ref_dev = _device_copy(st, "ref", enc)
            plan.align_chunk = enc.align_frames_per_chunk(n)
            if plan.align_chunk == 0:  # (one frame larger than the scratch: the host writers, on host-superposed frames)
                plan.pdb_chunk = plan.dcd_chunk = 0
        if self.torsions is not None:
            width = int(st.tor_index.shape[0])
            if width > 0 and int(st.tor_index.max()) >= n:
                raise ValueError(f"torsions: the molecule of {label!r} names atom {int(st.tor_index.max())}, the samples have {n} atoms")
            plan.tor_chunk = enc.features_frames_per_chunk(width)  # (0: no torsion, or one frame's torsions larger than the staging buffer)
            if plan.tor_chunk > 0:
                plan.tor_index_dev = _device_copy(st, "tor_index", enc)
        return plan

    def _host_fallbacks(self, st: _LabelState, enc, plan: _BatchPlan) -> Tuple[bool, bool]:
        """After a chain's jobs ran: does the host formatter write its (.pdb, .dcd) instead?  The .pdb when the device made none (no
        template, or one model larger than the staging buffer) or met a value the fixed PDB layout cannot hold (counted by the kernel);
        the .dcd when the device made none.  The joined file of that kind is then rewritten whole after the batch."""
        wants_pdb = self.write_pdb and st.mol is not None
        return (wants_pdb and (plan.pdb_chunk == 0 or enc.unencodable() != 0)), (self.write_dcd and plan.dcd_chunk == 0)

    def _write_batch_device(self, label: str, new: List[np.ndarray], all_chains: np.ndarray, start: int, block: torch.Tensor, ready) -> None:
        """The ``.pdb`` / ``.dcd`` and side files of a batch encoded on the GPU from ``block`` [chains, n, T, 3] (the device twin of ``new``):
        per chain its own files, and ``joined.pdb`` / ``joined.dcd`` extended by the chain's frames (models numbered on from the frames
        already there) instead of rewritten.  ``all_chains`` [n, chains so far * T, 3]: for the host formatter, should it have to."""
        st = self._states[label]
        if self._encoder is None or self._encoder.device != block.device:
            self._encoder = DeviceTrajectoryEncoder(block.device)
        enc = self._encoder
        enc.stream.wait_event(ready)
        T = int(block.shape[2])
        plan = self._plan(st, label, enc, int(block.shape[1]))
        joined = {ext: self.filename_pred(label, "joined", ext) for ext in ("pdb", "dcd")}
        if st.joined_frames == 0:  # files of an earlier run are replaced, as the host path does
            _unlink(joined.values())
        stale_pdb = stale_dcd = False
        for c, arr in enumerate(new):
            own = {ext: self.filename_pred(label, start + c, ext) for ext in ("pdb", "dcd")}
            _unlink(own.values())
            rmsd = np.empty(T, dtype=np.float32) if plan.align_chunk > 0 else None
            tor = np.empty((T, int(st.tor_index.shape[0])), dtype=np.float32) if plan.tor_chunk > 0 else None
            if plan.pdb_chunk > 0:
                enc.reset_unencodable()
            enc.run(_chain_jobs(enc, plan, block[c].transpose(0, 1), own, joined, st.joined_frames + c * T, rmsd, tor))
            if tor is None:  # (F = 0: [T, 0]; or the host formulas)
                tor = self._torsions_host(st, arr)
            if self.superpose and rmsd is None:
                rmsd = self._host_frames(st, arr)[1]
            self._save_chain_side_files(st, label, start + c, tor, rmsd)
            host_pdb, host_dcd = self._host_fallbacks(st, enc, plan)
            if host_pdb or host_dcd:
                self._save_host(st, label, start + c, self._host_frames(st, arr)[0], pdb=host_pdb, dcd=host_dcd)
            stale_pdb, stale_dcd = stale_pdb or host_pdb, stale_dcd or host_dcd
        if stale_pdb or stale_dcd:
            self._save_host(st, label, "joined", self._host_frames(st, all_chains)[0], pdb=stale_pdb, dcd=stale_dcd)
        self._save_joined_side_files(st, label)

    def _submit(self, fn, *args) -> None:
        if not self.async_write:  # a failed synchronous write surfaces at the next batch too, through the same gather
            from concurrent.futures import Future

            fut = Future()
            try:
                fut.set_result(fn(*args))
            except Exception as e:
                fut.set_exception(e)
            self._pending.append(fut)
            return
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor

            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="jamun-writer")
        self._pending.append(self._pool.submit(fn, *args))

    def flush(self) -> None:
        """Wait for the files of every batch handed over so far (errors of the writer thread surface here)."""
        t0 = time.perf_counter()
        pending, self._pending = self._pending, []
        for fut in pending:
            fut.result()
        self.wait_s += time.perf_counter() - t0

    def on_sample_end(self, sampler):
        try:
            self.flush()  # (the reference only uploads the joined files to wandb here, _save_trajectory.py:64-76: out of scope)
        finally:
            self.close()

    def close(self) -> None:
        """Stop the writer thread (also called by Sampler.sample when the loop raises: pending writes finish, their errors are not re-raised
        over the original one)."""
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
