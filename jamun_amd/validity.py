"""Chemical validity of sampled frames: the share of non-bonded atom pairs that clash and the share of bonds of a wrong length, per frame.

The reference's fourth per-trajectory sampler metric (``metrics/_chemical_validity.py``, ``callbacks/sampler/chemical_validity.yaml``).  A
non-bonded pair is an issue when its atoms are closer than ``(1 - tol)`` times the sum of their van der Waals radii, a bond when its length
lies outside ``(1 +- tol)`` times the sum of the covalent radii.  The reference walks all atom pairs in Python, which is why it looks at
100 frames of a chain; here every frame can be checked.

EVERY DECISION IS EXACT.  Frames are float32.  For a pair (i, j) the number compared is

    s = (dx*dx + dy*dy) + dz*dz        dx = x_j - x_i, every operation in float32, in this order, no contraction

which is what ``np.linalg.norm(..., axis=1)`` sums before its square root.  The reference decides ``d < thr`` and ``d > thr`` with
``d = fl32(sqrt(s))`` and a float64 ``thr``.  ``fl32(sqrt(.))`` is monotone and never lands on the midpoint of two float32 numbers (the
square of a midpoint has 50 significant bits, a float32 ``s`` has 24), so each decision is a comparison of ``s`` with ONE float32 number
made once on the host, `s_below` or `s_above`.  The kernel (``jamun_validity.hip``) therefore takes no square root, host and device do
the same IEEE multiplications, additions and comparisons, and their counts agree integer for integer.  NaN compares false on both sides
(a pair with a NaN difference is no issue, as in the reference); ``s = +inf`` is a bond issue and no clash, as in the reference.

    `s_below`, `s_above`                      the thresholds on the squared distance
    `validity_tables`                         the tables of a molecule: one clash threshold per atom pair, two per bond
    `validity_counts_host`                    the specification and the host path (numpy, float32)
    ``native.validity_counts``                the device path
    `ChemicalValidityMetrics`                 the meter `callbacks.TrajectoryMetricCallback` drives

Out of scope: the wandb tables and histograms of the reference's class.  Under several ranks each rank meters the walkers it owns and
rank 0 writes its own; the chains are not gathered.
"""

from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .meters import TrajectoryMeter, save_npz
from .native import VALIDITY_MAX_ATOMS

# The reference's two tables (nm), value for value.  Its covalent radius of sulphur, 1.005, is evidently a typo for 0.105; it is kept so that
# the default reproduces the reference's numbers (pass ``covalent_radii={"S": 0.105}`` to correct it).
VDW_RADII = {"C": 0.170, "O": 0.152, "N": 0.155, "H": 0.120, "F": 0.147, "S": 0.180, "other": 0.150}
COVALENT_RADII = {"C": 0.076, "O": 0.066, "N": 0.071, "H": 0.031, "F": 0.057, "S": 1.005, "other": 0.070}

_F32 = np.float32
_INF32 = np.float32(np.inf)


def _f32_at_least(v: float) -> np.float32:
    """The smallest float32 ``>= v`` (float64)."""
    f = _F32(v)
    return f if float(f) >= v else np.nextafter(f, _INF32)


def _f32_at_most(v: float) -> np.float32:
    """The largest float32 ``<= v`` (float64)."""
    f = _F32(v)
    return f if float(f) <= v else np.nextafter(f, -_INF32)


def s_below(thr: float) -> np.float32:
    """The float32 ``S`` with ``fl32(sqrt(s)) < thr  <=>  s < S`` for every float32 ``s >= 0`` (``thr`` a float64).  With ``c`` the smallest
    float32 ``>= thr`` and ``p`` its predecessor, ``d < thr`` means ``d <= p``, that is ``sqrt(s)`` below the midpoint of ``p`` and ``c``;
    ``S`` is the smallest float32 at or above the midpoint's square (exact in float64: 25 bits squared).  0 for ``thr <= 0``."""
    thr = float(thr)
    if not thr > 0.0:
        if math.isnan(thr):
            raise ValueError("a threshold must not be NaN")
        return _F32(0.0)
    if math.isinf(thr):
        return _INF32  # (every finite s is below; s = inf is not)
    c = _f32_at_least(thr)
    p = np.nextafter(c, -_INF32)
    mid = (float(p) + float(c)) / 2.0
    return _f32_at_least(mid * mid)


def s_above(thr: float) -> np.float32:
    """The float32 ``S`` with ``fl32(sqrt(s)) > thr  <=>  s > S`` for every float32 ``s >= 0`` (``thr`` a float64 ``>= 0``).  With ``q`` the
    largest float32 ``<= thr`` and ``u`` its successor, ``d > thr`` means ``d >= u``, that is ``sqrt(s)`` above the midpoint of ``q`` and
    ``u``; ``S`` is the largest float32 at or below the midpoint's square."""
    thr = float(thr)
    if math.isnan(thr) or thr < 0.0:
        raise ValueError(f"an upper threshold must be a number >= 0, got {thr}")
    if math.isinf(thr):
        return _INF32
    q = _f32_at_most(thr)
    u = np.nextafter(q, _INF32)
    if np.isinf(u):
        return q  # (thr at the top of the float32 range: only s = inf is above)
    mid = (float(q) + float(u)) / 2.0
    return _f32_at_most(mid * mid)


def _radii(defaults: dict, override: Optional[dict], what: str) -> dict:
    table = dict(defaults)
    for k, v in (override or {}).items():
        v = float(v)
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"{what}[{k!r}] must be a finite radius >= 0, got {v}")
        table[str(k)] = v
    return table


def _tolerance(v, name: str) -> float:
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"{name} must be finite and >= 0, got {v}")
    return v


def validity_tables(mol: dict, volume_exclusion_tolerance: float, bond_length_tolerance: float, vdw_radii: Optional[dict] = None,
                    covalent_radii: Optional[dict] = None) -> dict:
    """The tables `validity_counts_host` and ``native.validity_counts`` work from, for the molecule ``mol`` (``mol["elements"]``, one
    symbol per atom, and ``mol["bonds"]`` ``[2, B]``; a molecule without elements is a ``ValueError``):

        clash_s      float32 [n (n - 1) / 2]   the upper triangle in row-major (i < j) order: `s_below` of ``(1 - vtol) * (vdw_i + vdw_j)``,
                                               and 0 for a bonded pair (no s lies below 0: a bonded pair never clashes)
        bonds        int32 [B, 2]              normalised to (min, max), de-duplicated, sorted
        bond_lo_s    float32 [B]               `s_below` of ``(1 - btol) * (cov_i + cov_j)``
        bond_hi_s    float32 [B]               `s_above` of ``(1 + btol) * (cov_i + cov_j)``
        num_nonbonded_pairs, num_bonds         the two denominators, ``n (n - 1) / 2 - B`` and ``B``
        n_atoms, elements, vdw_radii, covalent_radii (the two tables used), volume_exclusion_tolerance, bond_length_tolerance

    The radii default to the reference's tables `VDW_RADII` and `COVALENT_RADII`, copied value for value: that includes its covalent radius
    of sulphur, 1.005 nm, evidently a typo for 0.105, so that the default reproduces the reference's numbers.  The two optional dicts
    override entries.  An element absent from a table takes its ``"other"`` entry; the reference has that entry but raises ``KeyError``
    (a documented, strictly more permissive deviation).  A bond of an atom with itself or with an index outside ``[0, n)`` is a
    ``ValueError``.  The reference excludes a bond from the clash test only if it is stored lower index first (as mdtraj and
    `pdb.read_pdb` store it); the normalisation makes that hold in general.  Tolerances must be finite and ``>= 0``."""
    elements = mol.get("elements")
    if elements is None:
        raise ValueError("validity_tables: the molecule has no 'elements' to look the radii up with")
    elements = [str(e) for e in elements]
    n = len(elements)
    if n < 1:
        raise ValueError("validity_tables: the molecule has no atoms")
    vtol = _tolerance(volume_exclusion_tolerance, "volume_exclusion_tolerance")
    btol = _tolerance(bond_length_tolerance, "bond_length_tolerance")
    vdw_table = _radii(VDW_RADII, vdw_radii, "vdw_radii")
    cov_table = _radii(COVALENT_RADII, covalent_radii, "covalent_radii")
    vdw = np.array([vdw_table.get(e, vdw_table["other"]) for e in elements], dtype=np.float64)
    cov = np.array([cov_table.get(e, cov_table["other"]) for e in elements], dtype=np.float64)

    raw = mol.get("bonds")
    raw = np.zeros((2, 0), dtype=np.int64) if raw is None else (raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw))
    if raw.size == 0:
        raw = np.zeros((2, 0), dtype=np.int64)
    if raw.dtype.kind not in "iu" or raw.ndim != 2 or raw.shape[0] != 2:
        raise ValueError(f"mol['bonds'] must be an integer [2, B] table, got {raw.dtype} {tuple(raw.shape)}")
    raw = raw.astype(np.int64).T
    bad = ((raw < 0) | (raw >= n)).any(axis=1) | (raw[:, 0] == raw[:, 1])
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError(f"bond {j}, {raw[j].tolist()}, is not two different atoms in [0, {n})")
    bonds = np.unique(np.sort(raw, axis=1), axis=0).reshape(-1, 2)  # (min, max), no duplicates, sorted by (i, j)
    B = int(bonds.shape[0])

    iu, ju = np.triu_indices(n, k=1)  # row-major (i < j)
    thr = (1.0 - vtol) * (vdw[iu] + vdw[ju])  # (float64, the reference's expression)
    distinct, inverse = np.unique(thr, return_inverse=True)  # (a handful: one per pair of elements)
    clash_s = np.array([s_below(t) for t in distinct.tolist()], dtype=np.float32)[inverse.reshape(-1)].reshape(-1)
    bi, bj = bonds[:, 0], bonds[:, 1]
    clash_s[bi * (2 * n - bi - 1) // 2 + (bj - bi - 1)] = 0.0
    cov_sum = cov[bi] + cov[bj]
    bond_lo_s = np.array([s_below(t) for t in ((1.0 - btol) * cov_sum).tolist()], dtype=np.float32).reshape(-1)
    bond_hi_s = np.array([s_above(t) for t in ((1.0 + btol) * cov_sum).tolist()], dtype=np.float32).reshape(-1)
    return {"clash_s": clash_s, "bonds": np.ascontiguousarray(bonds, dtype=np.int32), "bond_lo_s": bond_lo_s, "bond_hi_s": bond_hi_s,
            "num_nonbonded_pairs": n * (n - 1) // 2 - B, "num_bonds": B, "n_atoms": n, "elements": elements,
            "vdw_radii": vdw_table, "covalent_radii": cov_table, "volume_exclusion_tolerance": vtol, "bond_length_tolerance": btol}


HOST_BLOCK = 1 << 20  # (frame, pair) decisions the host path forms at a time


def validity_counts_host(frames, tables) -> Tuple[np.ndarray, np.ndarray]:
    """``frames [T, n, 3]`` and the tables of `validity_tables` -> ``(counts uint32 [T, 2], bond_frames uint32 [B])``: ``counts[t]`` =
    (clashes, bad bonds) of frame ``t``; ``bond_frames[b]`` = the number of frames in which bond ``b`` is off (it shows WHICH bond
    breaks).  The specification of ``jamun_validity_counts``: vectorised numpy in float32 (frames of another float type are rounded to
    float32 first), nothing is cast to float64, and a comparison of ``s`` with a NaN difference is false."""
    x = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    if x.ndim != 3 or x.shape[2] != 3 or x.dtype.kind != "f":
        raise ValueError(f"frames must be a floating-point [T, n, 3] array, got {x.dtype} {tuple(x.shape)}")
    x = x.astype(np.float32, copy=False)
    T, n = int(x.shape[0]), int(x.shape[1])
    clash_s, bonds = np.asarray(tables["clash_s"]), np.asarray(tables["bonds"]).reshape(-1, 2)
    lo, hi = np.asarray(tables["bond_lo_s"]), np.asarray(tables["bond_hi_s"])
    B = int(bonds.shape[0])
    if clash_s.dtype != np.float32 or lo.dtype != np.float32 or hi.dtype != np.float32:
        raise ValueError("the thresholds must be float32")
    if clash_s.shape != (n * (n - 1) // 2,) or lo.shape != (B,) or hi.shape != (B,):
        raise ValueError(f"the tables are not those of a molecule of {n} atoms and {B} bonds")
    if B and (bonds.min() < 0 or bonds.max() >= n):
        raise ValueError(f"a bond has an index outside [0, {n})")
    counts = np.zeros((T, 2), dtype=np.uint32)
    bond_frames = np.zeros((B,), dtype=np.uint32)
    step = max(1, HOST_BLOCK // max(n, B, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, T, step):
            xb = x[t0 : t0 + step]
            clashes = np.zeros(xb.shape[0], dtype=np.uint32)
            row = 0
            for i in range(n - 1):
                d = xb[:, i + 1 :, :] - xb[:, i : i + 1, :]
                s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                clashes += (s < clash_s[row : row + n - 1 - i]).sum(axis=1, dtype=np.uint32)
                row += n - 1 - i
            counts[t0 : t0 + step, 0] = clashes
            if B:
                d = xb[:, bonds[:, 1], :] - xb[:, bonds[:, 0], :]
                s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                assert s.dtype == np.float32
                off = (s < lo) | (s > hi)
                counts[t0 : t0 + step, 1] = off.sum(axis=1, dtype=np.uint32)
                bond_frames += off.sum(axis=0, dtype=np.uint32)
    return counts, bond_frames


def fractions(counts: np.ndarray, tables: dict) -> Tuple[np.ndarray, np.ndarray]:
    """``counts [K, 2]`` -> ``(volume_exclusion_issues, bond_length_issues)``, float64 ``[K]``: count / denominator, NaN where the
    denominator is 0 (a molecule whose every pair is bonded, a molecule without bonds; the reference divides by zero there)."""
    c = np.asarray(counts).astype(np.float64).reshape(-1, 2)
    den = (int(tables["num_nonbonded_pairs"]), int(tables["num_bonds"]))
    return tuple(c[:, k] / den[k] if den[k] > 0 else np.full(c.shape[0], np.nan) for k in (0, 1))


def frame_factor(T: int, num_molecules_per_trajectory: Optional[int]) -> int:
    """The reference's rule: the frames ``[::max(T // num_molecules_per_trajectory, 1)]`` of a trajectory of ``T`` are checked; ``None``
    checks every frame."""
    return 1 if num_molecules_per_trajectory is None else max(int(T) // int(num_molecules_per_trajectory), 1)


class ChemicalValidityMetrics(TrajectoryMeter):
    """The meter of one dataset (the ``TrajectoryMetric`` protocol `callbacks.TrajectoryMetricCallback` drives; the reference's
    ``ChemicalValidityMetrics``): per checked frame the share of clashing non-bonded pairs and of bonds of a wrong length, written under
    ``<output_dir>/<label>/chemical_validity/`` on rank 0:

        tables.json     elements, the radii used, tolerances, bonds, both denominators, the frame rule
        <i>.npz         per chain: frame_indices int64 [K], clash_counts and bond_counts uint32 [K], volume_exclusion_issues and
                        bond_length_issues float64 [K] (count / denominator; NaN where the denominator is 0), bond_frames uint32 [B] (the
                        checked frames in which bond b is off)
        joined.npz      the chains so far concatenated in running order, frame_indices offset as the frames of ``joined.npy`` are,
                        bond_frames summed
        true_traj.npz   the same arrays for the dataset's own frames ``dataset.xyz``, when it has them

    Frames: the reference's rule, ``frames[::max(T // num_molecules_per_trajectory, 1)]``; ``num_molecules_per_trajectory=None`` checks
    every frame, which is what the device path is for (on the device the selection is a strided view and costs nothing).

    ``device``: ``"auto"`` takes the device path (``native.validity_counts`` on the ``[T, n, 3]`` view of the chain; counts stay on the
    device until `compute`) for float32 sample tensors on a GPU when the native library loads and the molecule has at most
    ``native.VALIDITY_MAX_ATOMS`` atoms, else the host path `validity_counts_host`; both give the same integers.  ``"host"`` forces the
    host path, ``"device"`` makes a missing device path an error.

    `compute` returns, in the reference's keys, ``<label>/mean_volume_exclusion_issues/pred_traj_<i>`` and
    ``<label>/mean_bond_length_issues/pred_traj_<i>`` for the chains new since the last call, and the two ``.../true_traj`` keys when the
    dataset has frames of its own."""

    DIRECTORY = "chemical_validity"

    def __init__(self, dataset, volume_exclusion_tolerance: float, bond_length_tolerance: float,
                 num_molecules_per_trajectory: Optional[int] = 100, sample_key: str = "xhat_traj", output_dir: str = "sampler",
                 device: str = "auto", vdw_radii: Optional[dict] = None, covalent_radii: Optional[dict] = None, **_):
        super().__init__(dataset, sample_key, output_dir, device)
        k = num_molecules_per_trajectory
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1):
            raise ValueError(f"num_molecules_per_trajectory must be a positive integer or None, got {k!r}")
        mol = getattr(dataset, "molecule", None)
        if mol is None:
            raise ValueError(f"ChemicalValidityMetrics: the dataset of label {dataset.label()!r} has no molecule")
        self.num_molecules_per_trajectory = None if k is None else int(k)
        self.tables = validity_tables(mol, volume_exclusion_tolerance, bond_length_tolerance, vdw_radii, covalent_radii)
        self.n_atoms = int(self.tables["n_atoms"])
        self._joined: List[dict] = []  # per chain, on the host: frame_indices (offset), counts [K, 2], bond_frames [B]
        self._true: Optional[Dict[str, float]] = None

    def _device_fits(self) -> bool:
        return self.n_atoms <= VALIDITY_MAX_ATOMS

    def _device_needs(self) -> str:
        return (f"ChemicalValidityMetrics(device='device') needs float32 sample tensors on a GPU and a molecule of at most "
                f"{VALIDITY_MAX_ATOMS} atoms (this one has {self.n_atoms})")

    def _counts(self, frames):
        """Frames ``[K, n, 3]`` -> (counts [K, 2], bond_frames [B]): int32 device tensors on the device path, uint32 arrays on the host path."""
        if int(frames.shape[1]) != self.n_atoms:
            raise ValueError(f"the frames of {self.label!r} must have {self.n_atoms} atoms, got {tuple(frames.shape)}")
        if self._device_path(frames):
            from . import native

            if frames.device not in self._dev:
                self._dev[frames.device] = native.upload_validity_tables(self.tables, self.n_atoms, frames.device)
            return native.validity_counts(frames, self._dev[frames.device])
        return validity_counts_host(frames, self.tables)

    def _arrays(self, frame_indices: np.ndarray, counts, bond_frames) -> dict:
        """What an ``.npz`` here holds, from counts of either path (brought to the host)."""
        counts = counts.cpu().numpy().view(np.uint32) if torch.is_tensor(counts) else np.asarray(counts, dtype=np.uint32)
        bond_frames = bond_frames.cpu().numpy().view(np.uint32) if torch.is_tensor(bond_frames) else np.asarray(bond_frames, dtype=np.uint32)
        vol, bond = fractions(counts, self.tables)
        return {"frame_indices": np.asarray(frame_indices, dtype=np.int64), "clash_counts": np.ascontiguousarray(counts[:, 0]),
                "bond_counts": np.ascontiguousarray(counts[:, 1]), "volume_exclusion_issues": vol, "bond_length_issues": bond,
                "bond_frames": bond_frames}

    def _select(self, frames):
        """The checked frames of ``frames [T, n, 3]`` (a strided view) and their indices."""
        factor = frame_factor(int(frames.shape[0]), self.num_molecules_per_trajectory)
        return frames[::factor], np.arange(0, int(frames.shape[0]), factor, dtype=np.int64)

    def on_sample_start(self):
        write = self._is_rank_zero()
        ref = self._reference_frames(self.n_atoms, "the frames of the dataset")
        true = None
        if ref is not None:
            sub, idx = self._select(ref)
            true = self._arrays(idx, *self._counts(self._on_compute_device(sub)))
            self._true = {f"{self.label}/mean_volume_exclusion_issues/true_traj": float(np.mean(true["volume_exclusion_issues"])),
                          f"{self.label}/mean_bond_length_issues/true_traj": float(np.mean(true["bond_length_issues"]))}
        if not write:
            return
        d = self._dir()
        t = self.tables
        with open(os.path.join(d, "tables.json"), "w") as f:
            json.dump({"elements": t["elements"], "vdw_radii": t["vdw_radii"], "covalent_radii": t["covalent_radii"],
                       "volume_exclusion_tolerance": t["volume_exclusion_tolerance"], "bond_length_tolerance": t["bond_length_tolerance"],
                       "bonds": t["bonds"].tolist(), "num_nonbonded_pairs": t["num_nonbonded_pairs"], "num_bonds": t["num_bonds"],
                       "num_molecules_per_trajectory": self.num_molecules_per_trajectory,
                       "frame_rule": "every frame" if self.num_molecules_per_trajectory is None else
                       "frames[::max(T // num_molecules_per_trajectory, 1)]"}, f, indent=1)
        if true is not None:
            save_npz(os.path.join(d, "true_traj.npz"), **true)

    def update(self, sample) -> None:
        index, frames, off = self._next_chain(sample)
        T = int(frames.shape[0])
        if T == 0:
            return
        sub, idx = self._select(frames)
        counts, bond_frames = self._counts(sub)  # (on the device path: queued, nothing read back)
        self._pending.append({"index": index, "frame_indices": idx, "counts": counts, "bond_frames": bond_frames, "joined_at": off})
        self.joined_frames = off + T

    def compute(self) -> Dict[str, float]:
        """Brings the counts of the chains seen since the last call to the host, writes ``<i>.npz`` and ``joined.npz`` (rank 0) and
        returns the chains' mean fractions."""
        pending, write, d = self._take_pending()
        out: Dict[str, float] = {}
        for rec in pending:
            a = self._arrays(rec["frame_indices"], rec["counts"], rec["bond_frames"])
            self._joined.append({**a, "frame_indices": a["frame_indices"] + rec["joined_at"]})
            out[f"{self.label}/mean_volume_exclusion_issues/pred_traj_{rec['index']}"] = float(np.mean(a["volume_exclusion_issues"]))
            out[f"{self.label}/mean_bond_length_issues/pred_traj_{rec['index']}"] = float(np.mean(a["bond_length_issues"]))
            if write:
                save_npz(os.path.join(d, f"{rec['index']}.npz"), **a)
        if write and pending:
            joined = {k: np.concatenate([c[k] for c in self._joined]) for k in self._joined[0] if k != "bond_frames"}
            total = np.sum([c["bond_frames"].astype(np.uint64) for c in self._joined], axis=0)
            joined["bond_frames"] = np.asarray(total).astype(np.uint32).reshape(-1)
            save_npz(os.path.join(d, "joined.npz"), **joined)
        if self._true is not None:
            out.update(self._true)
        return out
