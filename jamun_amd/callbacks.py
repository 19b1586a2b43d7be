"""Sampler callbacks: trajectory writer, metric dispatch and timing.

``SaveTrajectoryCallback`` writes the file set of the reference's ``SaveTrajectory`` metric
(``/root/reference/src/jamun/metrics/_save_trajectory.py:17-30,53-56,78-97``, ``metrics/_utils.py:84-113``) under
``sampler/<label>/``:

    topology.pdb                                   first frame of the dataset            (on_sample_start)
    predicted_samples/npy/<i>.npy   [n, T, 3] nm   one per chain                         (every batch)
    predicted_samples/pdb/<i>.pdb, dcd/<i>.dcd     the same chain as PDB models / CHARMM DCD (Angstrom)
    predicted_samples/{npy,pdb,dcd}/joined.*       all chains so far, frames concatenated: [n, chains*T, 3]

``analysis/load_trajectory.py:88-107`` needs ``dcd/joined.dcd`` plus ``topology.pdb`` (or ``pdb/0.pdb``).  Samples are
dispatched by ``dataset_label`` (``callbacks/sampler/_utils.py:42-52``) and validated against the dataset
(``metrics/_utils.py:15-28``).  With several ranks the per-rank blocks are gathered to rank 0 once per batch and label
(``jamun_amd.dist.gather_ragged``) — what torchmetrics' ``dist_reduce_fx="cat"`` does in the reference.
"""

from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import dist
from .data import ATOM_TYPES


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
        labels = []
        self.datasets = {}
        for d in datasets:
            if d.label() not in self.datasets:
                labels.append(d.label())
                self.datasets[d.label()] = d
        self.labels = sorted(labels)
        self.sample_key = sample_key
        self.output_dir = output_dir
        self.write_pdb = write_pdb
        self.write_dcd = write_dcd
        self.save_true_trajectory = save_true_trajectory
        self.npy_index_restarts_per_batch = npy_index_restarts_per_batch
        self.chains: Dict[str, List[np.ndarray]] = {l: [] for l in self.labels}  # per label: list of [n, T, 3]
        self.num_chains_seen = {l: 0 for l in self.labels}
        # Files are written on ONE side thread, in submission order, while the next batch walks on the GPU (the walk is a single native call
        # that releases the GIL; numpy's file writes release it too): a 20 000-step batch of 256 dipeptides is 1 GB per key, and its files
        # take as long to write as the GPU needs for the walk.  on_sample_end (and flush) wait for the writer; wait_s is that time.
        self.async_write = bool(async_write)
        self._pool = None
        self._pending: list = []
        self.wait_s = 0.0
        from . import dist

        self._stager = dist.HostStager()  # one pinned + one device staging buffer for the whole run (dist.gather_ragged_to_host)
        self.gather_timings: Dict[str, float] = {}  # gather_s / gather_bytes accumulated over batches and labels (bench.py: e2e_sharded)
        self._encoder = None  # traj_encode.DeviceTrajectoryEncoder, created with the first device-encoded batch
        self._dev_blocks: dict = {}  # (label, first chain index) -> (device block [chains, n, T, 3], event recorded behind its producer)
        self._joined_frames = {l: 0 for l in self.labels}  # models / frames in joined.pdb / joined.dcd
        self.superpose = bool(superpose)
        self._ref: Dict[str, np.ndarray] = {}  # superpose: per label the reference structure [n, 3] (float32, nm)
        self._ref_dev: dict = {}  # ... and its device copy, made on the encoder's stream with the first device-encoded batch
        self._rmsd: Dict[str, List[np.ndarray]] = {l: [] for l in self.labels}  # ... and per chain the RMSD of its frames, [T] each
        if self.superpose:
            for label in self.labels:
                mol = getattr(self.datasets[label], "molecule", None)
                if mol is None or mol.get("pos") is None:
                    raise ValueError(f"SaveTrajectoryCallback(superpose=True): the dataset of label {label!r} has no molecule, so no reference "
                                     "structure to superpose on")
                pos = mol["pos"]
                self._ref[label] = np.ascontiguousarray(pos.detach().cpu().numpy() if torch.is_tensor(pos) else pos, dtype=np.float32)
        self._tor_index: Dict[str, np.ndarray] = {}  # torsions: per label the index table int32 [F, 4] ...
        self._tor_labels: Dict[str, List[str]] = {}  # ... the labels of its rows ...
        self._tor_index_dev: dict = {}  # ... its device copy, made on the encoder's stream with the first device-encoded batch
        self._tor: Dict[str, List[np.ndarray]] = {l: [] for l in self.labels}  # ... and per chain the torsions of its frames, [T, F] each
        if self.torsions is not None:
            from .features import torsion_indices

            for label in self.labels:
                mol = getattr(self.datasets[label], "molecule", None)
                if mol is None:
                    raise ValueError(f"SaveTrajectoryCallback(torsions={torsions!r}): the dataset of label {label!r} has no molecule to find torsions in")
                self._tor_index[label], self._tor_labels[label] = torsion_indices(mol, backbone=True, sidechain=self.torsions == "all")

    def _dir(self, label: str, ext: str) -> str:
        d = os.path.join(self.output_dir, label, "predicted_samples", ext)
        os.makedirs(d, exist_ok=True)
        return d

    def _mol(self, label: str) -> Optional[dict]:
        mol = getattr(self.datasets[label], "molecule", None)
        return mol if (mol is not None and "atom_names" in mol) else None

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

    def _torsions_host(self, label: str, frames: np.ndarray) -> np.ndarray:
        """frames [T, n, 3] (raw) -> their torsions float32 [T, F] on the host."""
        from .features import internal_coords_host

        return internal_coords_host(frames, self._tor_index[label]).astype(np.float32)

    def on_sample_start(self, sampler):
        if not sampler.is_global_zero:
            return
        from .pdb import save_pdb

        for label in self.labels:
            for ext in ("npy", "pdb", "dcd"):
                self._dir(label, ext)
            if self.torsions is not None:
                with open(os.path.join(self.output_dir, label, "torsion_labels.json"), "w") as f:
                    json.dump({"labels": self._tor_labels[label], "atom_indices": self._tor_index[label].tolist(), "unit": "rad"}, f, indent=1)
            mol = self._mol(label)
            if mol is not None and self.write_pdb:  # topology from the dataset's first frame (_save_trajectory.py:53-56)
                save_pdb(os.path.join(self.output_dir, label, "topology.pdb"), mol, mol["pos"][None])
            if self.save_true_trajectory:  # the dataset's own frames as true_samples/{pdb,dcd}/0.* (_save_trajectory.py:22-26,58-62)
                from .pdb import save_dcd

                ds = self.datasets[label]
                xyz = getattr(ds, "xyz", None)
                frames = (xyz if xyz is not None else mol["pos"][None]).detach().cpu().numpy() if mol is not None or xyz is not None else None
                if frames is not None:
                    for ext in ("pdb", "dcd"):
                        os.makedirs(os.path.join(self.output_dir, label, "true_samples", ext), exist_ok=True)
                    if mol is not None:
                        save_pdb(os.path.join(self.output_dir, label, "true_samples", "pdb", "0.pdb"), mol, frames)
                    save_dcd(os.path.join(self.output_dir, label, "true_samples", "dcd", "0.dcd"), frames)

    def _write_chain(self, label: str, index, arr: np.ndarray, npy_index=None) -> None:
        """arr [n, T, 3] nm -> <index>.npy / .pdb / .dcd"""
        from .pdb import save_dcd, save_pdb

        np.save(self.filename_pred(label, index if npy_index is None else npy_index, "npy"), arr)
        frames = np.transpose(arr, (1, 0, 2))  # "atoms frames coords -> frames atoms coords" (utils/mdtraj.py:17-21)
        if self.torsions is not None:  # (of the raw frames; joined = the chains' arrays, kept as _rmsd keeps them)
            if index != "joined":
                self._tor[label].append(self._torsions_host(label, frames))
            np.save(self.filename_torsions(label, index), np.concatenate(self._tor[label]) if index == "joined" else self._tor[label][-1])
        if self.superpose:  # (the .npy above stays the raw sampler output)
            frames, rmsd = self._superposed(label, frames)
            np.save(self.filename_rmsd(label, index), rmsd)
            if index != "joined":
                self._rmsd[label].append(rmsd)  # (kept per chain: a later batch on the device path extends rmsd/joined.npy from these)
        mol = self._mol(label)
        if self.write_pdb and mol is not None:
            save_pdb(self.filename_pred(label, index, "pdb"), mol, frames)
        if self.write_dcd:
            save_dcd(self.filename_pred(label, index, "dcd"), frames)

    def _superposed(self, label: str, frames: np.ndarray):
        """frames [T, n, 3] -> (the frames superposed on the label's reference structure, their RMSD to it [T]) on the host."""
        from .superpose import superpose_host

        return superpose_host(frames, self._ref[label])

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

    def _use_device_encoder(self, sample: Sequence[dict]) -> bool:
        if self.encode == "host":
            return False
        tensors = [s[self.sample_key] for s in sample if self.sample_key in s]
        if not tensors:
            return False  # (nothing to write)
        on_gpu = all(torch.is_tensor(t) and t.is_cuda for t in tensors)
        grouped = torch.distributed.is_available() and torch.distributed.is_initialized()
        if self.encode == "device":
            if not on_gpu:
                raise RuntimeError("SaveTrajectoryCallback(encode='device') needs the sample tensors on a GPU; use encode='host' (or 'auto') for CPU tensors")
            if grouped:
                raise RuntimeError("SaveTrajectoryCallback(encode='device') does not run under a process group: the trajectory gather delivers host blocks")
            from . import _lib

            _lib.load()
            return True
        if not on_gpu or grouped:
            return False
        from . import _lib

        return _lib.available()

    def on_after_sample_batch(self, sample: Sequence[dict], sampler):
        error = self._finished_writer_error()
        use_device = self._use_device_encoder(sample) and (self.write_dcd or self.write_pdb or self.torsions is not None)
        for s in sample:
            if s.get("dataset_label") not in self.datasets:
                raise KeyError(f"sample dataset label {s.get('dataset_label')!r} has no dataset")
        for label in self.labels:
            mine = [s for s in sample if s.get("dataset_label") == label]
            for s in mine:
                validate_sample(s, self.datasets[label])
                if s[self.sample_key].ndim != 3:
                    raise ValueError(f"Invalid sample shape: {tuple(s[self.sample_key].shape)}, expected (num_atoms, num_frames, 3).")
            # a rank without walkers of this label contributes nothing; gather_ragged agrees on the trailing shape first
            block = torch.stack([s[self.sample_key] for s in mine]).contiguous() if mine else None  # [chains_local, n, T, 3]
            # one block at a time through ONE reusable device receive buffer and ONE reusable pinned staging buffer; what the writer
            # thread (and self.chains) keep are pageable copies
            blocks = dist.gather_ragged_to_host(block, dst=0, device=sampler.device, stager=self._stager, timings=self.gather_timings,
                                                error=error)
            if blocks is None:
                continue
            start = self.num_chains_seen[label]
            self.num_chains_seen[label] = start + sum(int(b.shape[0]) for b in blocks)
            if use_device and block is not None and block.is_cuda and block.dtype == torch.float32 and block.shape[0] > 0 and block.shape[2] > 0:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(block.device))
                self._dev_blocks[(label, start)] = (block, ready)  # kept alive until the writer thread has encoded it
            self._submit(self._write_batch, label, blocks, start)
        if error is not None:  # (no label, so no gather to carry it)
            raise error

    def _write_batch(self, label: str, blocks: List[np.ndarray], start: int) -> None:
        dev = self._dev_blocks.pop((label, start), None)
        new = [c for b in blocks for c in b]
        self.chains[label].extend(new)
        if dev is not None:
            self._write_batch_device(label, new, start, *dev)
        else:
            for i, arr in enumerate(new, start=start):
                self._write_chain(label, i, arr, npy_index=(i - start) if self.npy_index_restarts_per_batch else None)
            if self.chains[label]:
                self._write_chain(label, "joined", np.concatenate(self.chains[label], axis=1))  # "b n t c -> n (b t) c"
        self._joined_frames[label] = sum(int(c.shape[1]) for c in self.chains[label])

    def _write_batch_device(self, label: str, new: List[np.ndarray], start: int, block: torch.Tensor, ready) -> None:
        """The files of `_write_batch` with ``.pdb`` / ``.dcd`` bytes encoded on the GPU from ``block`` [chains, n, T, 3] (the device
        twin of ``new``): per chain its own files, and ``joined.pdb`` / ``joined.dcd`` extended by the chain's frames (models
        numbered on from the frames already there) instead of rewritten.  A file with a value the fixed PDB layout cannot hold
        (counted by the kernel) is rewritten by `save_pdb`."""
        from .pdb import append_dcd_frames, append_pdb_models, save_dcd, save_pdb
        from .traj_encode import DeviceTrajectoryEncoder

        for i, arr in enumerate(new, start=start):
            np.save(self.filename_pred(label, (i - start) if self.npy_index_restarts_per_batch else i, "npy"), arr)
        np.save(self.filename_pred(label, "joined", "npy"), np.concatenate(self.chains[label], axis=1))  # (axis 1: cannot be appended)
        if self._encoder is None or self._encoder.device != block.device:
            self._encoder = DeviceTrajectoryEncoder(block.device)
        enc = self._encoder
        enc.stream.wait_event(ready)
        n, T = int(block.shape[1]), int(block.shape[2])
        mol = self._mol(label) if self.write_pdb else None
        tmpl = None
        if mol is not None and len(mol["atom_names"]) == n and n + 1 <= 99999:
            try:
                tmpl = enc.template(mol)
            except UnicodeEncodeError:
                tmpl = None
        pdb_chunk = enc.pdb_frames_per_chunk(int(tmpl[0].numel())) if tmpl is not None else 0
        dcd_chunk = enc.dcd_frames_per_chunk(n) if self.write_dcd else 0
        joined_pdb, joined_dcd = self.filename_pred(label, "joined", "pdb"), self.filename_pred(label, "joined", "dcd")
        joined_at = self._joined_frames[label]
        if joined_at == 0:  # files of an earlier run are replaced, as the host path does
            for path in (joined_pdb, joined_dcd):
                if os.path.exists(path):
                    os.unlink(path)
        def host_frames(arr):  # [n, T, 3] -> [T, n, 3] for the host writers: superposed when the device frames are
            frames = np.transpose(arr, (1, 0, 2))
            return self._superposed(label, frames)[0] if self.superpose else frames

        joined_pdb_stale = False
        ref_dev, align_chunk = None, 0
        if self.superpose:
            if self._ref[label].shape[0] != n:
                raise ValueError(f"superpose: the reference structure of {label!r} has {self._ref[label].shape[0]} atoms, the samples have {n}")
            if self._ref_dev.get(label) is None or self._ref_dev[label].device != enc.device:
                with torch.cuda.device(enc.device), torch.cuda.stream(enc.stream):
                    self._ref_dev[label] = torch.from_numpy(self._ref[label]).to(enc.device)
            ref_dev = self._ref_dev[label]
            align_chunk = enc.align_frames_per_chunk(n)
            if align_chunk == 0:  # (one frame larger than the scratch: the host writers, on host-superposed frames)
                pdb_chunk = dcd_chunk = 0

        tor_index_dev, tor_width, tor_chunk = None, 0, 0
        if self.torsions is not None:
            tor_width = int(self._tor_index[label].shape[0])
            if tor_width > 0 and int(self._tor_index[label].max()) >= n:
                raise ValueError(f"torsions: the molecule of {label!r} names atom {int(self._tor_index[label].max())}, the samples have {n} atoms")
            tor_chunk = enc.features_frames_per_chunk(tor_width)  # (0: no torsion, or one frame's torsions larger than the staging buffer)
            if tor_chunk > 0:
                if self._tor_index_dev.get(label) is None or self._tor_index_dev[label].device != enc.device:
                    with torch.cuda.device(enc.device), torch.cuda.stream(enc.stream):
                        self._tor_index_dev[label] = torch.from_numpy(self._tor_index[label]).to(enc.device)
                tor_index_dev = self._tor_index_dev[label]

        def both(*sinks):
            def sink(data):
                for fn in sinks:
                    fn(data)
            return sink

        for c, (i, arr) in enumerate(enumerate(new, start=start)):
            frames = block[c].transpose(0, 1)  # [T, n, 3] view of the chain
            own_pdb, own_dcd = self.filename_pred(label, i, "pdb"), self.filename_pred(label, i, "dcd")
            for path in (own_pdb, own_dcd):
                if os.path.exists(path):
                    os.unlink(path)
            jobs = []
            spans = [(0, T, frames)]  # (first frame, end, the [end - first, n, 3] device view the encoders read)
            rmsd = None
            if align_chunk > 0:  # superposed chunk by chunk into the encoder's scratch; the RMSD leaves as the chunk's bytes
                rmsd = np.empty(T, dtype=np.float32)
                spans = [(s0, min(T, s0 + align_chunk), enc.align_view(n, min(T, s0 + align_chunk) - s0)) for s0 in range(0, T, align_chunk)]

                def keep_rmsd(data, a, b, r=rmsd):
                    r[a:b] = np.frombuffer(data, dtype=np.float32)

            if pdb_chunk > 0:
                enc.reset_unencodable()
            for s0, s1, view in spans:
                if rmsd is not None:
                    jobs.append((enc.superpose(frames[s0:s1], ref_dev, view), lambda data, a=s0, b=s1: keep_rmsd(data, a, b)))
                if pdb_chunk > 0:
                    for t0 in range(s0, s1, pdb_chunk):
                        t1 = min(s1, t0 + pdb_chunk)
                        jobs.append((enc.encode_pdb(view[t0 - s0 : t1 - s0], t0, *tmpl), lambda data, p=own_pdb: append_pdb_models(p, data)))
                        jobs.append((enc.encode_pdb(view[t0 - s0 : t1 - s0], joined_at + t0, *tmpl), lambda data: append_pdb_models(joined_pdb, data)))
                if dcd_chunk > 0:
                    for t0 in range(s0, s1, dcd_chunk):
                        t1 = min(s1, t0 + dcd_chunk)
                        jobs.append((enc.encode_dcd(view[t0 - s0 : t1 - s0]), both(lambda data, p=own_dcd, k=t1 - t0: append_dcd_frames(p, n, data, k),
                                                                                 lambda data, k=t1 - t0: append_dcd_frames(joined_dcd, n, data, k))))
            tor = None
            if tor_chunk > 0:  # torsions of the RAW chain, chunk by chunk straight into the staging buffer
                tor = np.empty((T, tor_width), dtype=np.float32)

                def keep_tor(data, a, b, dst=tor):
                    dst[a:b] = np.frombuffer(data, dtype=np.float32).reshape(b - a, tor_width)

                for t0 in range(0, T, tor_chunk):
                    t1 = min(T, t0 + tor_chunk)
                    jobs.append((enc.features(frames[t0:t1], tor_index_dev), lambda data, a=t0, b=t1, fn=keep_tor: fn(data, a, b)))
            enc.run(jobs)
            if self.torsions is not None:
                if tor is None:  # (F = 0: [T, 0]; or the host formulas)
                    tor = self._torsions_host(label, np.transpose(arr, (1, 0, 2)))
                np.save(self.filename_torsions(label, i), tor)
                self._tor[label].append(tor)
            if self.superpose:
                if rmsd is None:
                    rmsd = self._superposed(label, np.transpose(arr, (1, 0, 2)))[1]
                np.save(self.filename_rmsd(label, i), rmsd)
                self._rmsd[label].append(rmsd)
            if pdb_chunk > 0 and enc.unencodable() != 0:
                save_pdb(own_pdb, mol, host_frames(arr))
                joined_pdb_stale = True
            elif mol is not None and pdb_chunk == 0:  # (no template, or one model larger than the staging buffer: the host formatter)
                save_pdb(own_pdb, mol, host_frames(arr))
                joined_pdb_stale = True
            if self.write_dcd and dcd_chunk == 0:
                save_dcd(own_dcd, host_frames(arr))
            joined_at += T
        if joined_pdb_stale:
            save_pdb(joined_pdb, mol, host_frames(np.concatenate(self.chains[label], axis=1)))
        if self.write_dcd and dcd_chunk == 0:
            save_dcd(joined_dcd, host_frames(np.concatenate(self.chains[label], axis=1)))
        if self.superpose:
            np.save(self.filename_rmsd(label, "joined"), np.concatenate(self._rmsd[label]))
        if self.torsions is not None:
            np.save(self.filename_torsions(label, "joined"), np.concatenate(self._tor[label]))

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
