"""The sliced Wasserstein distance of the Ramachandran descriptors of sampled frames from those of a reference trajectory, as the samples grow.

The reference's second curve (``metrics/_ramachandran.py:152-174,195-203``, beside the JS divergence of `ramachandran`): per frame the
descriptor ``[cos phi..., sin phi..., cos psi..., sin psi...]``, and ``ot.sliced_wasserstein_distance(descriptors, ref_descriptors,
n_projections=20)`` for the first k samples, k = 100, 200, 400, ... and all samples, per chain and for the joined trajectory.  That call is a
projection of both clouds on random unit directions, per direction the 1-D Wasserstein distance at p = 2 with uniform weights, and
``(mean over directions of W2^2) ** 0.5``; none of it needs the ``ot`` package:

    `projections`, `descriptor_rows`, `project_host`, `order_image`, `sort_segments_host`,    the specification (numpy, float64) and the
    `merge_sorted_host`, `w2sq_sorted_host`, `sliced_wasserstein_host`                        host path
    ``native.swd_project``, ``native.swd_sort_segments``, ``native.swd_merge``,               the device path (``jamun_swd.hip``): keys and
    ``native.swd_w2sq``                                                                       sorted columns equal the specification's bit
                                                                                              for bit, W2^2 within (n + m) 2^-52 relative
    `SlicedWassersteinMetrics`                                                                the meter `callbacks.TrajectoryMetricCallback` drives

REPRODUCIBLE.  The reference passes no seed, so POT draws new directions at every call and its number cannot be reproduced.  Here the
directions are `projections` ``(d, n_projections, seed)``: ``np.random.RandomState(seed).randn(d, L)`` with unit columns, which is what POT
draws when it is handed that ``RandomState``; they are written beside the results.

A KEY is ``fl32(sum_j float64(x[t, j]) * float64(proj[j, l]))``, the sum in float64 in column order.  The product of two promoted float32
values has at most 48 significant bits and is exact in float64, so a fused and an unfused accumulate give the same bits: that is what
makes the keys reproducible bit for bit on the device.

SORTED means sorted by `order_image`, a map float32 -> uint32 that preserves the order of the reals, with ``-0.0 < +0.0`` and every NaN
last as the quiet NaN ``0x7FC00000``: a sorted column is unique as bits, whatever algorithm produced it.

W2^2 of two sorted columns of n and m keys is the exact quantile integral on the integer grid of n m cells (`w2sq_sorted_host`).  POT's
``wasserstein_1d`` evaluates the same integral with float cumulative sums of 1 / n; parity with ``ot`` itself is unpinned, because it is
not installed (as pyemma is not for `tica` and `msm`): the specification was checked against a brute force (``np.repeat``) to 2e-15
relative and against a transcription of ``wasserstein_1d`` to 3e-13 relative for (n, m) from (1, 1) to (1000, 999).

Out of scope: the plots and wandb tables.  Under several ranks each rank meters the walkers it owns and rank 0 writes its own.
"""

from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from .features import internal_coords_host
from .meters import TrajectoryMeter, save_npz
from .native import SWD_MAX_PROJ, SWD_MAX_WIDTH, check_cuts
from .ramachandran import phi_psi_pairs, sample_counts

NAN_IMAGE = np.uint32(0xFFFFFFFF)
QUIET_NAN_BITS = np.uint32(0x7FC00000)


def _array(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)


def projections(d: int, n_projections: int = 20, seed: int = 0) -> np.ndarray:
    """float32 ``[d, L]``: ``np.random.RandomState(seed).randn(d, L)``, each column divided by its Euclidean norm in float64, then rounded
    to float32: the directions POT's ``get_random_projections`` draws from that ``RandomState``.  The reference passes no seed and is not
    reproducible; this is."""
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1:
        raise ValueError(f"d must be a positive integer, got {d!r}")
    if isinstance(n_projections, bool) or not isinstance(n_projections, (int, np.integer)) or n_projections < 1:
        raise ValueError(f"n_projections must be a positive integer, got {n_projections!r}")
    p = np.random.RandomState(seed).randn(int(d), int(n_projections))
    return (p / np.sqrt(np.sum(p * p, axis=0, keepdims=True))).astype(np.float32)


def descriptor_rows(n_phi: int, n_psi: int) -> np.ndarray:
    """int64 ``[2 (n_phi + n_psi)]``: for every interleaved column ``(cos, sin)`` of ``internal_coords(cossin=True)`` on the phi-then-psi
    table of `ramachandran.phi_psi_pairs`, its column in the reference's descriptor ``[cos phi..., sin phi..., cos psi..., sin psi...]``.
    Row ``j`` of a projection matrix means the reference's column ``j``; ``proj[descriptor_rows(...)]`` is the matrix for the interleaved
    columns."""
    rows = []
    for f in range(n_phi + n_psi):
        for is_sin in (0, 1):
            rows.append(f + is_sin * n_phi if f < n_phi else 2 * n_phi + (f - n_phi) + is_sin * n_psi)
    return np.array(rows, dtype=np.int64)


def project_host(x, proj) -> np.ndarray:
    """``x [T, W]`` float32, ``proj [W, L]`` float32 -> float32 ``[L, T]``: element ``(l, t)`` is the float64 sum, taken in column order
    ``j = 0 ... W - 1`` onto +0.0, of ``float64(x[t, j]) * float64(proj[j, l])``, rounded once to float32.  Every product is exact in
    float64.  The specification of ``jamun_swd_project``."""
    x, proj = _array(x), _array(proj)
    if x.ndim != 2 or proj.ndim != 2 or x.dtype != np.float32 or proj.dtype != np.float32 or proj.shape[0] != x.shape[1]:
        raise ValueError(f"x must be float32 [T, W] and proj float32 [W, L], got {x.dtype} {x.shape} and {proj.dtype} {proj.shape}")
    acc = np.zeros((proj.shape[1], x.shape[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(x.shape[1]):
            acc = acc + proj[j].astype(np.float64)[:, None] * x[:, j].astype(np.float64)[None, :]
        return acc.astype(np.float32)


def order_image(keys) -> np.ndarray:
    """float32 -> uint32 of the same shape, preserving the order of the reals: all bits of a negative flipped, the sign bit of a
    non-negative set, every NaN (of either sign) sent to ``0xFFFFFFFF``.  So ``-0.0 < +0.0`` and NaN comes last."""
    k = np.ascontiguousarray(_array(keys))
    if k.dtype != np.float32:
        raise ValueError(f"keys must hold float32, got {k.dtype}")
    b = k.view(np.uint32)
    image = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), NAN_IMAGE, image).astype(np.uint32)


def keys_of_image(image) -> np.ndarray:
    """The inverse of `order_image`; ``0xFFFFFFFF`` gives the quiet NaN ``0x7FC00000``."""
    i = np.ascontiguousarray(image, dtype=np.uint32)
    b = np.where(i & np.uint32(0x80000000), i ^ np.uint32(0x80000000), ~i)
    return np.where(i == NAN_IMAGE, QUIET_NAN_BITS, b).astype(np.uint32).view(np.float32)


def _columns(name: str, a) -> np.ndarray:
    a = _array(a)
    if a.ndim != 2 or a.dtype != np.float32 or a.shape[1] < 1:
        raise ValueError(f"{name} must be float32 [L, n] with n >= 1, got {a.dtype} {a.shape}")
    return a


def sort_segments_host(keys, bounds) -> np.ndarray:
    """``keys [L, T]`` float32, ``bounds`` as `native.check_cuts` takes them (1 to 64 cuts ascending strictly within ``[1, T]``) -> float32
    ``[L, T]``: of every column the frames ``cuts[c-1] <= t < cuts[c]`` sorted by `order_image`, each segment on its own; frames from the
    last cut on are copied as they are.  The specification of ``jamun_swd_sort_segments``."""
    k = _columns("keys", keys)
    cuts = check_cuts(bounds, k.shape[1])
    out = k.copy()
    start = 0
    for c in cuts.tolist():
        out[:, start:c] = keys_of_image(np.sort(order_image(k[:, start:c]), axis=1))
        start = c
    return out


def merge_sorted_host(a, b) -> np.ndarray:
    """Sorted ``a [L, n]`` and ``b [L, m]`` -> sorted float32 ``[L, n + m]``.  The specification of ``jamun_swd_merge``."""
    a, b = _columns("a", a), _columns("b", b)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a and b must have the same number of rows, got {a.shape} and {b.shape}")
    return keys_of_image(np.sort(np.concatenate([order_image(a), order_image(b)], axis=1), axis=1))


def w2sq_sorted_host(u, v) -> np.ndarray:
    """Sorted ``u [L, n]`` and ``v [L, m]`` (float32) -> float64 ``[L]``: the quantile integral of ``(F^-1(q) - G^-1(q))^2`` over
    ``[0, 1]`` for uniform weights, exactly.  On the integer grid of ``n m`` cells ``u``'s cell ``i`` is ``[i m, (i + 1) m)`` and ``v``'s cell
    ``j`` is ``[j n, (j + 1) n)``; the pieces are the intervals between consecutive members of ``{i m} | {j n}``, and a piece in cells
    ``(i, j)`` of integer length ``w`` contributes ``w * (float64(u_i) - float64(v_j))^2`` (a difference, a square, a product, each rounded
    once).  The sum is divided by ``n m``.  At most ``n + m - 1`` non-negative terms: any order of summation is within ``(n + m) 2^-52``
    relative.  A non-finite key follows IEEE and makes that row's value non-finite.  The specification of ``jamun_swd_w2sq``."""
    u, v = _columns("u", u), _columns("v", v)
    if u.shape[0] != v.shape[0]:
        raise ValueError(f"u and v must have the same number of rows, got {u.shape} and {v.shape}")
    n, m = int(u.shape[1]), int(v.shape[1])
    edges = np.union1d(np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n)
    lo, w = edges[:-1], np.diff(edges)
    with np.errstate(invalid="ignore", over="ignore"):
        d = u[:, lo // m].astype(np.float64) - v[:, lo // n].astype(np.float64)
        return ((d * d) * w.astype(np.float64)[None, :]).sum(axis=1) / float(n * m)


def distance_of(w2sq) -> float:
    """``(mean over directions of W2^2) ** 0.5``."""
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.mean(np.asarray(w2sq, dtype=np.float64))))


def sliced_wasserstein_host(x, y, proj) -> float:
    """The sliced Wasserstein distance of the descriptor rows ``x [T, W]`` and ``y [M, W]`` (float32) on the directions ``proj [W, L]``:
    `project_host`, a sort of each, `w2sq_sorted_host`, `distance_of`."""
    kx, ky = project_host(x, proj), project_host(y, proj)
    return distance_of(w2sq_sorted_host(sort_segments_host(kx, [kx.shape[1]]), sort_segments_host(ky, [ky.shape[1]])))


class SlicedWassersteinMetrics(TrajectoryMeter):
    """The meter of one dataset (the ``TrajectoryMetric`` protocol `callbacks.TrajectoryMetricCallback` drives): per chain and for the
    joined trajectory the curve sliced Wasserstein distance against the number of samples, written under
    ``<output_dir>/<label>/sliced_wasserstein/`` on rank 0:

        projections.npz   projections float32 [d, L] (row j: the reference's descriptor column j), descriptor_rows, seed, pairing,
                          torsion_labels, reference_frames, and a note where there is nothing to compute
        <i>.npz           per chain: num_samples [C] (`ramachandran.sample_counts`), ws_distance [C], w2sq_per_projection [C, L],
                          nonfinite [C] (the frames among the first num_samples with a non-finite descriptor)
        joined.npz        the same for all chains so far in running order, frames concatenated

    The reference frames come from ``reference`` (frames ``[T, n, 3]``, or the path of such an ``.npy``) if given, else from the dataset's
    own ``xyz``; with neither (or a molecule without phi and psi) there is nothing to compute: ``projections.npz`` says so and no
    distances are written.  `on_sample_start` projects and sorts them once, `REFERENCE_CHUNK` frames at a time with the chunks merged,
    and keeps the sorted ``[L, M]`` columns where the samples are computed.

    Per chain the cuts are its own `sample_counts` and the joined trajectory's cuts that fall inside it, as `RamachandranMetrics.update`
    forms them: the chain is projected, its segments are sorted, the sorted prefix grows by one merge per cut, W2^2 against the reference is
    evaluated at every cut of the chain's own counts, and at a joined cut the prefix is first merged with the sorted columns of the chains
    joined so far.  After the chain it is merged into those.  The kept state is ``4 L`` bytes per joined frame (and per reference frame).

    A frame with a non-finite descriptor is counted in ``nonfinite``; its NaN keys sort last, and a prefix that contains such a frame
    reports a NaN distance: nothing is dropped silently.

    ``device``: ``"auto"`` takes the device path for float32 sample tensors on a GPU when the native library loads, ``d <= 128`` and
    ``L <= 64`` (``native.internal_coords`` with ``cossin``, ``native.swd_project``, ``swd_sort_segments``, ``swd_merge``, ``swd_w2sq``; only
    the W2^2 values and the counts come back), else the host path: the specification on ``internal_coords_host(..., cossin=True)
    .astype(float32)``.  ``"host"`` forces the host path, ``"device"`` makes a missing device path an error.  `compute` returns
    ``{"<label>/ws_distance/pred_traj_joined": the joined trajectory's last value}``."""

    DIRECTORY = "sliced_wasserstein"
    REFERENCE_CHUNK = 1 << 20  # frames of the reference trajectory projected and sorted at a time

    def __init__(self, dataset, sample_key: str = "xhat_traj", n_projections: int = 20, seed: int = 0, pairing: str = "reference",
                 reference=None, output_dir: str = "sampler", device: str = "auto", **_):
        super().__init__(dataset, sample_key, output_dir, device)
        if isinstance(n_projections, bool) or not isinstance(n_projections, (int, np.integer)) or n_projections < 1:
            raise ValueError(f"n_projections must be a positive integer, got {n_projections!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
        mol = getattr(dataset, "molecule", None)
        if mol is None:
            raise ValueError(f"SlicedWassersteinMetrics: the dataset of label {dataset.label()!r} has no molecule to find phi and psi in")
        self.n_projections, self.seed, self.pairing, self.reference = int(n_projections), int(seed), pairing, reference
        self.n_atoms = len(mol["atom_names"])
        self.index, _, _ = phi_psi_pairs(mol, pairing)  # (all phi, then all psi; the pairing decides only whether unequal counts are an error)
        from .features import torsion_indices

        _, labels = torsion_indices(mol, backbone=True, sidechain=False)
        self.torsion_labels = [l for l in labels if l.startswith("PHI ")] + [l for l in labels if l.startswith("PSI ")]
        n_phi = sum(l.startswith("PHI ") for l in self.torsion_labels)
        self.width = 2 * len(self.torsion_labels)
        self.rows = descriptor_rows(n_phi, len(self.torsion_labels) - n_phi)
        self.proj = projections(self.width, self.n_projections, self.seed) if self.width else np.zeros((0, self.n_projections), np.float32)
        self.proj_rows = np.ascontiguousarray(self.proj[self.rows])  # for the interleaved columns
        self.ref_sorted = None       # [L, M], an array or a device tensor
        self.joined_sorted = None    # [L, joined frames], likewise
        self.joined_nonfinite = 0
        self._joined_at: Dict[int, tuple] = {}  # joined cut 100 * 2^i -> (W2^2 [L], non-finite frames) of the first that many joined frames
        self._last_joined: Optional[float] = None

    def _device_fits(self) -> bool:
        return 1 <= self.width <= SWD_MAX_WIDTH and self.n_projections <= SWD_MAX_PROJ

    def _device_needs(self) -> str:
        return "SlicedWassersteinMetrics(device='device') needs float32 sample tensors on a GPU, at most 128 descriptor columns and at most 64 projections"

    # ---- the four operations on either path: device tensors in, device tensors out; arrays likewise ---------------------------------------

    def _uploaded(self, dev):
        if dev not in self._dev:  # (index, projection matrix)
            self._dev[dev] = [torch.from_numpy(self.index).to(dev), torch.from_numpy(self.proj_rows).to(dev)]
        return self._dev[dev]

    def _keys(self, frames):
        """Raw frames ``[T, n, 3]`` -> (keys [L, T], per frame whether a descriptor is non-finite [T])."""
        if self._device_path(frames):
            from . import native

            index, proj = self._uploaded(frames.device)
            x = native.internal_coords(frames, index, cossin=True)
            return native.swd_project(x, proj), ~torch.isfinite(x).all(dim=1)
        x = internal_coords_host(frames, self.index, cossin=True).astype(np.float32)
        return project_host(x, self.proj_rows), ~np.isfinite(x).all(axis=1)

    @staticmethod
    def _like(a, b):
        """``a`` where ``b`` is: on ``b``'s device if ``b`` is a tensor, else an array."""
        if torch.is_tensor(b):
            return a.to(b.device) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(b.device)
        return _array(a)

    @staticmethod
    def _sort(keys, cuts):
        if torch.is_tensor(keys):
            from . import native

            return native.swd_sort_segments(keys, np.asarray(cuts, dtype=np.int32))
        return sort_segments_host(keys, np.asarray(cuts, dtype=np.int64))

    def _merge(self, a, b):
        if a is None:
            return b
        if torch.is_tensor(b):
            from . import native

            return native.swd_merge(self._like(a, b), b)
        return merge_sorted_host(self._like(a, b), b)

    def _w2sq(self, u):
        if torch.is_tensor(u):
            from . import native

            self.ref_sorted = self._like(self.ref_sorted, u)
            return native.swd_w2sq(u, self.ref_sorted)
        return w2sq_sorted_host(u, self._like(self.ref_sorted, u))

    # ---- protocol ------------------------------------------------------------------------------------------------------------------------

    def on_sample_start(self):
        ref = self._reference_frames(self.n_atoms, "the reference frames of", self.reference) if self.width else None
        if ref is not None:
            for t0 in range(0, int(ref.shape[0]), self.REFERENCE_CHUNK):
                chunk = self._on_compute_device(ref[t0 : t0 + self.REFERENCE_CHUNK])
                keys, _ = self._keys(chunk)
                self.ref_sorted = self._merge(self.ref_sorted, self._sort(keys, [int(chunk.shape[0])]))
        if not self._is_rank_zero():
            return
        note = ("" if self.ref_sorted is not None else "the molecule has no phi or psi angle: nothing to compute, no distances are written" if not self.width
                else "no reference frames (neither dataset.xyz nor reference=): nothing to compute, no distances are written")
        save_npz(os.path.join(self._dir(), "projections.npz"), projections=self.proj, descriptor_rows=self.rows, seed=np.int64(self.seed),
                 pairing=np.array(self.pairing), torsion_labels=np.array(self.torsion_labels, dtype=np.str_),
                 reference_frames=np.int64(0 if self.ref_sorted is None else self.ref_sorted.shape[1]), note=np.array(note))

    def update(self, sample) -> None:
        index, frames, off = self._next_chain(sample)
        T = int(frames.shape[0])
        if T == 0 or self.ref_sorted is None:
            return
        own = sample_counts(T)
        inside = [100 * 2 ** i - off for i in range(10) if off < 100 * 2 ** i <= off + T]  # the joined trajectory's cuts, in local frames
        cuts = sorted(set(own) | set(inside))
        keys, bad = self._keys(frames)
        seg = self._sort(keys, cuts)
        bad_before = bad.cumsum(0)  # non-finite frames among the first t + 1
        prefix, start, w2, nonfinite = None, 0, [], []
        for c in cuts:
            prefix = self._merge(prefix, seg[:, start:c])
            start = c
            if c in own:
                w2.append(self._w2sq(prefix))
                nonfinite.append(bad_before[c - 1])
            if c in inside:
                self._joined_at[off + c] = (self._w2sq(self._merge(self.joined_sorted, prefix)), bad_before[c - 1] + self.joined_nonfinite)
        lib = torch if torch.is_tensor(seg) else np
        self.joined_sorted = self._merge(self.joined_sorted, prefix)  # (the last cut is the whole chain)
        self.joined_nonfinite = bad_before[T - 1] + self.joined_nonfinite
        self.joined_frames = off + T
        self._pending.append({"index": index, "num_samples": own, "w2sq": lib.stack(w2), "nonfinite": lib.stack(nonfinite)})

    @staticmethod
    def _curve(num_samples, w2sq, nonfinite) -> Dict[str, np.ndarray]:
        w2sq, nonfinite = np.asarray(w2sq, dtype=np.float64), np.asarray(nonfinite, dtype=np.int64)
        ws = np.array([float("nan") if k else distance_of(row) for row, k in zip(w2sq, nonfinite.tolist())], dtype=np.float64)
        return {"num_samples": np.asarray(num_samples, dtype=np.int64), "ws_distance": ws, "w2sq_per_projection": w2sq, "nonfinite": nonfinite}

    def compute(self) -> Dict[str, float]:
        """Brings the W2^2 values of the chains seen since the last call to the host, writes ``<i>.npz`` and ``joined.npz`` (rank 0) and
        returns the joined trajectory's last distance."""
        pending, write, d = self._take_pending()
        key = f"{self.label}/ws_distance/pred_traj_joined"
        for rec in pending:
            if write:
                save_npz(os.path.join(d, f"{rec['index']}.npz"), **self._curve(rec["num_samples"], _array(rec["w2sq"]), _array(rec["nonfinite"])))
        if not pending or self.joined_sorted is None:
            return {} if self._last_joined is None else {key: self._last_joined}
        cuts = sample_counts(self.joined_frames)
        at = [self._joined_at[g] if g != self.joined_frames else (self._w2sq(self.joined_sorted), self.joined_nonfinite) for g in cuts]
        out = self._curve(cuts, np.stack([_array(w) for w, _ in at]), [int(_array(k)) for _, k in at])
        self._last_joined = float(out["ws_distance"][-1])
        if write:
            save_npz(os.path.join(d, "joined.npz"), **out)
        return {key: self._last_joined}
