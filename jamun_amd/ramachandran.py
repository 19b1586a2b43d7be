"""Ramachandran histograms of sampled frames and their Jensen-Shannon divergence from a reference trajectory, as the samples grow.

The reference judges a sampling run by one curve (``metrics/_ramachandran.py:131-149,177-192``): the JS divergence between the (phi, psi)
histogram of the first k samples and that of the true trajectory, for k = 100, 200, 400, ... and all samples, per chain and for the joined
trajectory.  This module is that curve without mdtraj, scipy or matplotlib:

    `sample_counts`, `phi_psi_pairs`, `histogram_host`, `js_divergence_host`   the specification (numpy, float64) and the host path
    ``native.hist2d_pairs``, ``native.js_divergence`` (``jamun_hist.hip``)     the device path: counts equal the specification's integer
                                                                               for integer on the same float32 angles
    `RamachandranMetrics`                                                      the meter `callbacks.TrajectoryMetricCallback` drives

A histogram over frames ``[0, k)`` for several k is kept as SEGMENT histograms (frames ``cuts[c-1] <= t < cuts[c]``); the histogram of a
prefix is the integer sum of its segments, so nothing is counted twice and a joined trajectory is summed from its chains' counts.

Out of scope: the plots, the animations and the wandb tables of the reference's ``RamachandranPlotMetrics``.  Its second curve, the
sliced Wasserstein distance, is `swd.SlicedWassersteinMetrics` (a meter of its own: this one is unchanged).  Under several ranks each rank meters the walkers it owns and rank 0 writes its own; the chains
are not gathered.
"""

from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .features import internal_coords_host, torsion_indices
from .meters import TrajectoryMeter, save_npz  # noqa: F401  (save_npz: importable from here as before)
from .native import HIST_MAX_BINS, HIST_MAX_CUTS as MAX_CUTS, check_cuts


def sample_counts(T: int) -> List[int]:
    """``100 * 2**i`` for ``i < 10`` while strictly less than ``T``, then ``T``: the sample counts at which the reference evaluates a
    trajectory of ``T`` frames (``_num_subsamples_sequence_for_trajectory``)."""
    T = int(T)
    return [100 * 2 ** i for i in range(10) if 100 * 2 ** i < T] + [T]


def phi_psi_pairs(mol: dict, pairing: str = "reference") -> Tuple[np.ndarray, np.ndarray, List[str]]:
    """``(index int32 [F, 4], pairs int32 [P, 2], labels)``: the phi and psi rows of `features.torsion_indices` (all phi, then all psi) and
    the column pairs (phi column, psi column) that are histogrammed together, one label per pair.

    ``"reference"`` pairs the i-th phi with the i-th psi by running number, which is what the reference's ``phi_angles.flatten(),
    psi_angles.flatten()`` does: with mdtraj's rule (phi needs the previous residue, psi the next) that is phi of residue i + 1 with psi of
    residue i, so a dipeptide has one pair.  Unequal counts are a ``ValueError``.  ``"residue"`` pairs phi and psi of the same residue, the
    textbook plot; a dipeptide has none."""
    if pairing not in ("reference", "residue"):
        raise ValueError(f"pairing must be 'reference' or 'residue', got {pairing!r}")
    index, labels = torsion_indices(mol, backbone=True, sidechain=False)
    phi = [j for j, l in enumerate(labels) if l.startswith("PHI ")]
    psi = [j for j, l in enumerate(labels) if l.startswith("PSI ")]
    keep = phi + psi
    index = np.ascontiguousarray(index[keep], dtype=np.int32).reshape(-1, 4)
    labels = [labels[j] for j in keep]
    n_phi, n_psi = len(phi), len(psi)
    if pairing == "reference":
        if n_phi != n_psi:
            raise ValueError(f"pairing='reference' pairs the i-th phi with the i-th psi, but the molecule has {n_phi} phi and {n_psi} psi angles")
        pairs = [(i, n_phi + i) for i in range(n_phi)]
    else:  # phi = (C-, N, CA, C) and psi = (N, CA, C, N+) of one residue share N, CA, C
        psi_of = {tuple(index[n_phi + k, 0:3].tolist()): n_phi + k for k in range(n_psi)}
        pairs = [(i, psi_of[tuple(index[i, 1:4].tolist())]) for i in range(n_phi) if tuple(index[i, 1:4].tolist()) in psi_of]
    pair_labels = [f"{labels[a]} / {labels[b]}" for a, b in pairs]
    return index, np.array(pairs, dtype=np.int32).reshape(-1, 2), pair_labels


def histogram_host(angles, pairs, bins: int, cuts) -> Tuple[np.ndarray, np.ndarray]:
    """``angles [T, W]`` (radians, any float type), ``pairs [P, 2]`` (x column, y column), ``cuts`` (1 to 64 frame counts, strictly ascending
    in ``[1, T]``) -> ``(counts uint32 [C, P, bins, bins], skipped int64 [C, P])``: SEGMENT ``c`` holds the frames ``cuts[c-1] <= t <
    cuts[c]`` (``cuts[-1] := 0``).  The specification of ``jamun_hist2d_pairs``.

    The rule of a bin is numpy's, on the angle promoted to float64: edges ``e = np.linspace(-pi, pi, bins + 1)``, bin
    ``searchsorted(e, a, "right") - 1``, the last edge inclusive, with one addition: the angle is clipped to ``[-pi, pi]`` first.
    ``float32(pi) > pi``, so ``np.histogram2d`` drops a dihedral of exactly 180 degrees as atan2f returns it; clipped, it lies in the last
    bin (-180 degrees in the first).  A frame whose x or y is not finite is counted in ``skipped`` and in no bin."""
    a = np.asarray(angles.detach().cpu().numpy() if torch.is_tensor(angles) else angles)
    if a.ndim != 2:
        raise ValueError(f"angles must have shape [T, W], got {a.shape}")
    T, W = a.shape
    p = np.asarray(pairs)
    if p.size == 0:
        p = p.reshape(-1, 2).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu" or ((p < 0) | (p >= W)).any():
        raise ValueError(f"pairs must be an integer [P, 2] table of columns in [0, {W}), got {p.dtype} {p.shape}")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
        raise ValueError(f"bins must be a positive integer, got {bins!r}")
    bins = int(bins)
    c = check_cuts(cuts, T)
    edges = np.linspace(-np.pi, np.pi, bins + 1)
    counts = np.zeros((c.shape[0], p.shape[0], bins, bins), dtype=np.uint32)
    skipped = np.zeros((c.shape[0], p.shape[0]), dtype=np.int64)
    starts = np.concatenate([[0], c[:-1]])

    def bin_of(v):
        b = np.searchsorted(edges, np.clip(v, -np.pi, np.pi), side="right") - 1
        return np.minimum(b, bins - 1)  # (the last edge is inclusive)

    for j, (cx, cy) in enumerate(p.tolist()):
        x, y = a[:, cx].astype(np.float64), a[:, cy].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        flat = bin_of(np.where(ok, x, 0.0)) * bins + bin_of(np.where(ok, y, 0.0))
        for s, (t0, t1) in enumerate(zip(starts.tolist(), c.tolist())):
            m = ok[t0:t1]
            counts[s, j] = np.bincount(flat[t0:t1][m], minlength=bins * bins).reshape(bins, bins)
            skipped[s, j] = (t1 - t0) - int(m.sum())
    return counts, skipped


def _jsd(n: np.ndarray, r: np.ndarray) -> float:
    N, R = float(n.sum()), float(r.sum())
    if N == 0.0:
        return float("nan")
    p, q = n.astype(np.float64).ravel() / N, r.astype(np.float64).ravel() / R
    m = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        left = np.where(p > 0, p * np.log(np.where(p > 0, p / m, 1.0)), 0.0)
        right = np.where(q > 0, q * np.log(np.where(q > 0, q / m, 1.0)), 0.0)
    return 0.5 * float((left + right).sum())


def js_divergence_host(counts, ref_counts) -> Dict[str, np.ndarray]:
    """Segment counts ``[C, P, B, B]`` and reference counts ``[P, B, B]`` or ``[B, B]`` (one reference for every pair) ->
    ``{"pooled": float64 [C], "per_pair": float64 [C, P]}``: the Jensen-Shannon divergence, in nats with ``0 log 0 = 0``
    (``scipy.spatial.distance.jensenshannon(p, q) ** 2``, as the reference computes it), between the normalised histogram of the
    first ``cuts[c]`` frames (the PREFIX sum of the segments) and the normalised reference.  ``pooled`` sums all pairs into one
    histogram first (and the reference's pairs likewise): the reference's number.  A prefix without a counted frame gives NaN; a
    reference without a count is a ``ValueError``.  The specification of ``jamun_js_divergence``."""
    n = np.asarray(counts.detach().cpu().numpy() if torch.is_tensor(counts) else counts)
    r = np.asarray(ref_counts.detach().cpu().numpy() if torch.is_tensor(ref_counts) else ref_counts)
    if n.ndim != 4 or n.shape[2] != n.shape[3]:
        raise ValueError(f"counts must have shape [C, P, B, B], got {n.shape}")
    C, P, B = n.shape[0], n.shape[1], n.shape[2]
    if r.shape not in ((P, B, B), (B, B)):
        raise ValueError(f"ref_counts must have shape [{P}, {B}, {B}] or [{B}, {B}], got {r.shape}")
    if (n < 0).any() or (r < 0).any():
        raise ValueError("counts must not be negative")
    prefix = np.cumsum(n.astype(np.uint64), axis=0)
    r = r.astype(np.uint64)
    r_pooled = r.sum(axis=0) if r.ndim == 3 else r
    if int(r_pooled.sum()) == 0 or (r.ndim == 3 and (r.reshape(P, -1).sum(axis=1) == 0).any()):
        raise ValueError("the reference histogram has no count")
    pooled = np.array([_jsd(prefix[c].sum(axis=0), r_pooled) for c in range(C)], dtype=np.float64)
    per_pair = np.array([[_jsd(prefix[c, p], r[p] if r.ndim == 3 else r) for p in range(P)] for c in range(C)], dtype=np.float64).reshape(C, P)
    return {"pooled": pooled, "per_pair": per_pair}


class RamachandranMetrics(TrajectoryMeter):
    """The meter of one dataset (the ``TrajectoryMetric`` protocol `callbacks.TrajectoryMetricCallback` drives): per chain and for the
    joined trajectory the (phi, psi) histograms and the curve JS divergence against the number of samples, written under
    ``<output_dir>/<label>/ramachandran/`` on rank 0:

        pairs.json      labels and atom indices of the torsions, the pairs, pairing, bins, and whether a reference histogram exists
        true_traj.npz   counts [P, B, B] of the reference histogram (only with a reference)
        <i>.npz         per chain: counts uint32 [P, B, B] (all frames), num_samples [C] (`sample_counts`), skipped int64 [P], and with a
                        reference js_divergence [C] (pooled: the reference's number) and js_divergence_per_pair [C, P]
        joined.npz      the same for all chains so far in running order, frames concatenated (as ``joined.npy`` is); its counts are
                        integer sums of the chains' segment counts, never recomputed from frames

    The reference histogram comes from ``reference`` (frames ``[T, n, 3]``, or the path of such an ``.npy``) if given, else from the dataset's
    own frames ``dataset.xyz``; with neither, histograms are written, the JSD entries are omitted and ``pairs.json`` says so.

    ``device``: ``"auto"`` takes the device path for float32 sample tensors on a GPU when the native library loads and ``bins <= 128``
    (torsions of the RAW frames from ``native.internal_coords`` on the ``[T, n, 3]`` view of the chain, one ``native.hist2d_pairs`` call
    whose cuts are the chain's own `sample_counts` and the joined trajectory's cuts that fall inside the chain, ``native.js_divergence``;
    the angles stay on the device, only counts and JSD values come back), else the host path: the specification fed with
    ``internal_coords_host(...).astype(float32)``.  ``"host"`` forces the host path, ``"device"`` makes a missing device path an error.
    `compute` returns ``{"<label>/js_divergence/pred_traj_joined": the joined trajectory's last pooled value}``.

    Out of scope: plots, animations and wandb; the sliced Wasserstein distance of the reference's class is `swd.SlicedWassersteinMetrics`."""

    DIRECTORY = "ramachandran"

    def __init__(self, dataset, sample_key: str = "xhat_traj", bins: int = 100, pairing: str = "reference", reference=None,
                 output_dir: str = "sampler", device: str = "auto", **_):
        super().__init__(dataset, sample_key, output_dir, device)
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
            raise ValueError(f"bins must be a positive integer, got {bins!r}")
        mol = getattr(dataset, "molecule", None)
        if mol is None:
            raise ValueError(f"RamachandranMetrics: the dataset of label {dataset.label()!r} has no molecule to find phi and psi in")
        self.bins = int(bins)
        self.pairing = pairing
        self.reference = reference
        self.n_atoms = len(mol["atom_names"])
        self.index, self.pairs, self.pair_labels = phi_psi_pairs(mol, pairing)
        _, self.torsion_labels = torsion_indices(mol, backbone=True, sidechain=False)
        self.torsion_labels = [l for l in self.torsion_labels if l.startswith(("PHI ", "PSI "))]
        self.ref_counts: Optional[np.ndarray] = None  # uint32 [P, B, B]
        P, B = int(self.pairs.shape[0]), self.bins
        self.joined_counts = np.zeros((P, B, B), dtype=np.uint64)
        self.joined_skipped = np.zeros((P,), dtype=np.int64)
        self._joined_prefix: Dict[int, np.ndarray] = {}  # joined cut 100 * 2^i -> counts of the first that many joined frames
        self._last_joined: Optional[float] = None

    def _device_fits(self) -> bool:
        return self.bins <= HIST_MAX_BINS

    def _device_needs(self) -> str:
        return "RamachandranMetrics(device='device') needs float32 sample tensors on a GPU and bins <= 128"

    def _device_path(self, t) -> bool:
        return self.pairs.shape[0] > 0 and super()._device_path(t)  # (no pair: nothing to count on either path)

    def _uploaded(self, dev):
        if dev not in self._dev:  # (index, pairs, ref counts)
            self._dev[dev] = [torch.from_numpy(self.index).to(dev), torch.from_numpy(self.pairs).to(dev), None]
        if self._dev[dev][2] is None and self.ref_counts is not None:  # (the reference histogram itself is made with the first two)
            self._dev[dev][2] = torch.from_numpy(self.ref_counts.view(np.int32)).to(dev)
        return self._dev[dev]

    def _segments(self, frames, cuts: List[int]):
        """Raw frames ``[T, n, 3]`` -> (segment counts [C, P, B, B], skipped [C, P]) for ``cuts``: device tensors (int32) on the device
        path, arrays on the host path."""
        if self._device_path(frames):
            from . import native

            index, pairs, _ = self._uploaded(frames.device)
            angles = native.internal_coords(frames, index)
            return native.hist2d_pairs(angles, pairs, self.bins, np.asarray(cuts, dtype=np.int32))
        angles = internal_coords_host(frames, self.index).astype(np.float32)
        return histogram_host(angles, self.pairs, self.bins, np.asarray(cuts, dtype=np.int64))

    def _divergence(self, segments):
        """Segment counts -> (pooled [C], per_pair [C, P]) against the reference: device tensors in, device tensors out; arrays likewise."""
        if torch.is_tensor(segments):
            from . import native

            return native.js_divergence(segments, self._uploaded(segments.device)[2])
        d = js_divergence_host(segments, self.ref_counts)
        return d["pooled"], d["per_pair"]

    REFERENCE_CHUNK = 1 << 20  # frames of the reference trajectory histogrammed at a time

    def on_sample_start(self):
        P, B = int(self.pairs.shape[0]), self.bins
        ref = self._reference_frames(self.n_atoms, "the reference frames of", self.reference)
        if ref is not None and P > 0:
            total = np.zeros((P, B, B), dtype=np.uint64)
            for t0 in range(0, int(ref.shape[0]), self.REFERENCE_CHUNK):
                chunk = self._on_compute_device(ref[t0 : t0 + self.REFERENCE_CHUNK])
                counts, _ = self._segments(chunk, [int(chunk.shape[0])])
                counts = counts.cpu().numpy().view(np.uint32) if torch.is_tensor(counts) else counts
                total += counts[0]
            if int(total.sum()) > 0:  # (a chunk has fewer than 2^31 frames; the sum fits uint32 below 2^32 reference frames)
                self.ref_counts = total.astype(np.uint32)
        if not self._is_rank_zero():
            return
        d = self._dir()
        with open(os.path.join(d, "pairs.json"), "w") as f:
            json.dump({"torsion_labels": self.torsion_labels, "atom_indices": self.index.tolist(), "pairs": self.pairs.tolist(),
                       "pair_labels": self.pair_labels, "pairing": self.pairing, "bins": self.bins, "range": [-np.pi, np.pi],
                       "js_divergence": self.ref_counts is not None,
                       "note": None if self.ref_counts is not None else
                       "no reference frames (neither dataset.xyz nor reference=): histograms only, the js_divergence entries are omitted"}, f, indent=1)
        if self.ref_counts is not None:
            save_npz(os.path.join(d, "true_traj.npz"), counts=self.ref_counts)

    def update(self, sample) -> None:
        index, frames, off = self._next_chain(sample)
        T = int(frames.shape[0])
        if T == 0 or self.pairs.shape[0] == 0:
            return
        own = sample_counts(T)
        inside = [100 * 2 ** i - off for i in range(10) if off < 100 * 2 ** i <= off + T]  # the joined trajectory's cuts, in local frames
        cuts = sorted(set(own) | set(inside))
        seg, skipped = self._segments(frames, cuts)
        lib = torch if torch.is_tensor(seg) else np
        rows = [cuts.index(k) for k in own]
        rec = {"index": index, "num_samples": own, "counts": seg.sum(0), "skipped": skipped.sum(0), "joined_at": off, "frames": T,
               "prefix": {off + k: seg[: cuts.index(k) + 1].sum(0) for k in inside}}
        if self.ref_counts is not None:
            pooled, per_pair = self._divergence(seg)
            take = torch.tensor(rows, device=seg.device) if lib is torch else rows
            rec["pooled"], rec["per_pair"] = pooled[take], per_pair[take]
        self.joined_frames = off + T
        self._pending.append(rec)

    @staticmethod
    def _host(a, dtype=None):
        a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return a if dtype is None else a.astype(dtype)

    def compute(self) -> Dict[str, float]:
        """Brings the counts and JSD values of the chains seen since the last call to the host, adds them to the joined trajectory, writes
        ``<i>.npz`` and ``joined.npz`` (rank 0) and returns the joined trajectory's last pooled JSD."""
        pending, write, d = self._take_pending()
        gpu = None
        for rec in pending:
            if torch.is_tensor(rec["counts"]):
                gpu = rec["counts"].device
            counts = self._host(rec["counts"]).astype(np.int64).astype(np.uint32)  # (int32 carrying uint32 on the device path)
            skipped = self._host(rec["skipped"], np.int64)
            for g, pre in rec["prefix"].items():
                self._joined_prefix[g] = self.joined_counts + self._host(pre).astype(np.int64).astype(np.uint64)
            self.joined_counts = self.joined_counts + counts
            self.joined_skipped = self.joined_skipped + skipped
            if write:
                out = {"counts": counts, "num_samples": np.asarray(rec["num_samples"], dtype=np.int64), "skipped": skipped}
                if "pooled" in rec:
                    out["js_divergence"] = self._host(rec["pooled"], np.float64)
                    out["js_divergence_per_pair"] = self._host(rec["per_pair"], np.float64)
                save_npz(os.path.join(d, f"{rec['index']}.npz"), **out)
        if not pending or self.joined_frames == 0:
            return {} if self._last_joined is None else {f"{self.label}/js_divergence/pred_traj_joined": self._last_joined}
        cuts = sample_counts(self.joined_frames)
        prefix = [self._joined_prefix[g] if g != self.joined_frames else self.joined_counts for g in cuts]
        out = {"counts": self.joined_counts.astype(np.uint32), "num_samples": np.asarray(cuts, dtype=np.int64), "skipped": self.joined_skipped}
        if self.ref_counts is not None:
            seg = np.stack([prefix[0]] + [b - a for a, b in zip(prefix, prefix[1:])])  # the segments between the joined cuts
            if gpu is not None and int(seg.max()) < 2 ** 31:
                pooled, per_pair = self._divergence(torch.from_numpy(seg.astype(np.int32)).to(gpu))
            else:
                pooled, per_pair = self._divergence(seg)
            out["js_divergence"], out["js_divergence_per_pair"] = self._host(pooled, np.float64), self._host(per_pair, np.float64)
            self._last_joined = float(out["js_divergence"][-1])
        if write:
            save_npz(os.path.join(d, "joined.npz"), **out)
        return {} if self._last_joined is None else {f"{self.label}/js_divergence/pred_traj_joined": self._last_joined}
