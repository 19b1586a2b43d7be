"""Time-lagged independent component analysis (TICA) of sampled trajectories: whether a sampler finds the slow modes of the true dynamics.

The slow-mode part of the reference's analysis pipeline (``analysis/utils.py``: ``compute_TICA``, ``compute_TICA_stats``,
``compute_autocorrelation_stats``, driven from ``analysis/run_analysis.py``): a TICA model is fitted on the cos / sin torsion features of
the TRUE trajectory (pyemma's ``tica(lag=1000, kinetic_map=True)``), the sampled trajectory is projected on its components, and three
numbers are reported: the Jensen-Shannon distance of the histograms of the first component, of the first two components, and the
autocovariance of the first component (statsmodels' ``acovf(adjusted=True, demean=False)``).  Neither pyemma nor statsmodels is needed
here: the algorithm is pyemma's as documented, written out below.

    `lagged_moments_host`, `project_host`, `autocov_sums_host`   the specification (numpy, float64) and the host path of the three
                                                                 reductions over frames
    ``native.lagged_moments``, ``native.project_frames``, ``native.autocov_sums`` (``jamun_tica.hip``)   the device path: each output within
                                                                 the rounding of its additions of the specification, the same bits in every run
    `fit_tica`                                                   moments -> mean, eigenvalues, eigenvectors (host: two symmetric eigenproblems
                                                                 of the size of a feature row)
    `js_distance_host`                                           scipy's ``jensenshannon`` (the distance, not its square) without scipy
    `TICAMetrics`                                                the meter `callbacks.TICAMetricsCallback` drives

Features: interleaved (cos, sin) pairs of phi and psi of every residue and, with ``features="all"``, of chi1..chi4: what pyemma's
``add_backbone_torsions(cossin=True)`` and ``add_sidechain_torsions(cossin=True)`` give (`features.torsion_indices` without its omega rows,
``internal_coords(cossin=True)``).

k-means and the Markov state model of ``compute_MSM_stats`` are `jamun_amd.msm`'s.  Out of scope: plots, wandb, histograms of the components on the device, and
gathering chains across ranks (each rank meters its own walkers, as the other meters do).
"""

from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .features import internal_coords_host, torsion_indices
from .meters import TrajectoryMeter, save_npz
from .native import TICA_MAX_ACF_LAG, TICA_MAX_WIDTH


def _as_numpy(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ---- the specification of the three reductions ----------------------------------------------------------------------------------------------

def lagged_moments_host(x, lag: int) -> Tuple[np.ndarray, np.ndarray]:
    """``x [T, W]`` (any float type) and ``1 <= lag < T`` -> ``(sums float64 [2, W], moments float64 [3, W, W])`` over the ``N = T - lag``
    pairs ``(x_t, x_{t+lag})``: ``sums = (sum x_t, sum x_{t+lag})``, ``moments = (G, H, K)`` with ``G = sum x_t x_t^T``,
    ``H = sum x_{t+lag} x_{t+lag}^T``, ``K = sum x_t x_{t+lag}^T`` (row = the earlier frame; not symmetrised).  Every value is promoted to
    float64 first.  The specification of ``jamun_lagged_moments``."""
    x = np.asarray(_as_numpy(x), dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"expected x [T, W], got {x.shape}")
    T = x.shape[0]
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag < T:
        raise ValueError(f"lag must be an integer in [1, {T}) for {T} frames, got {lag!r}")
    a, b = x[: T - lag], x[lag:]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([a.sum(axis=0), b.sum(axis=0)]), np.stack([a.T @ a, b.T @ b, a.T @ b])


def project_host(x, mean, v) -> np.ndarray:
    """``out[t] = (x[t] - mean) @ v`` in float64: ``x [T, W]``, ``mean [W]``, ``v [W, d]`` -> ``[T, d]``.  The specification of
    ``jamun_project_frames``."""
    x = np.asarray(_as_numpy(x), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x - np.asarray(mean, dtype=np.float64)[None, :]) @ np.asarray(v, dtype=np.float64)


def autocov_sums_host(y, max_lag: int) -> np.ndarray:
    """``y [T]`` -> float64 ``[max_lag + 1]``: ``out[k] = sum_{t < T - k} y[t] y[t + k]``, 0 for ``k >= T``.  Divided by ``T - k`` it is
    statsmodels' ``acovf(y, adjusted=True, demean=False)``.  The specification of ``jamun_autocov_sums``."""
    y = np.asarray(_as_numpy(y), dtype=np.float64).reshape(-1)
    T = y.shape[0]
    out = np.zeros(int(max_lag) + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(min(int(max_lag) + 1, T)):
            out[k] = np.dot(y[: T - k], y[k:])
    return out


def autocov_from_sums(sums: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """``sums / counts`` where a lag has a pair, NaN where it has none."""
    sums, counts = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts > 0, sums / np.where(counts > 0, counts, 1.0), np.nan)


def autocov_counts(T: int, max_lag: int) -> np.ndarray:
    """The pairs behind each lag of a trajectory of ``T`` frames: ``max(T - k, 0)``, int64 ``[max_lag + 1]``."""
    return np.maximum(int(T) - np.arange(int(max_lag) + 1, dtype=np.int64), 0)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------

def fit_tica(sums, moments, n_pairs: int, epsilon: float = 1e-6, var_cutoff: float = 0.95, kinetic_map: bool = True) -> Dict[str, np.ndarray]:
    """The TICA model of the moments ``sums [2, W]`` / ``moments [3, W, W]`` of `lagged_moments_host` over ``n_pairs`` lag pairs.  Moments
    of several trajectories are SUMMED before the call (and their pairs counted together), so that no pair crosses from one trajectory
    into the next: pyemma's rule for a list of trajectories.  The reversible estimator:

        mu    = (s_0 + s_tau) / 2N
        C_0   = (G + H) / 2N - mu mu^T
        C_tau = (K + K^T) / 2N - mu mu^T

    ``C_0 = Q diag(s) Q^T``; the eigenvalues ``s > epsilon`` are kept, ``L = Q s^-1/2`` whitens; ``L^T C_tau L = R diag(lambda) R^T`` with
    the eigenvalues descending; the eigenvectors are ``U = L R``, scaled by their eigenvalues with ``kinetic_map``; the first ``d``
    components are kept, the smallest ``d`` whose cumulative ``sum lambda^2 / total`` reaches ``var_cutoff``.  Each eigenvector's entry of
    largest magnitude is made positive.  Returns ``mean [W]``, ``eigenvalues [m]`` (all kept by ``epsilon``), ``eigenvectors [W, d]``,
    ``cumulative_variance [m]`` and ``d``.  A ``ValueError`` where the moments are not finite or no eigenvalue of ``C_0`` passes ``epsilon``."""
    s = np.asarray(sums, dtype=np.float64)
    m = np.asarray(moments, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 2 or m.shape != (3, s.shape[1], s.shape[1]):
        raise ValueError(f"expected sums [2, W] and moments [3, W, W], got {s.shape} and {m.shape}")
    if n_pairs < 1:
        raise ValueError(f"n_pairs must be positive, got {n_pairs}")
    if not (np.isfinite(s).all() and np.isfinite(m).all()):
        raise ValueError("the moments are not finite")
    two_n = 2.0 * float(n_pairs)
    mu = (s[0] + s[1]) / two_n
    c0 = (m[0] + m[1]) / two_n - np.outer(mu, mu)
    ct = (m[2] + m[2].T) / two_n - np.outer(mu, mu)
    c0 = 0.5 * (c0 + c0.T)
    sv, q = np.linalg.eigh(c0)
    order = np.argsort(-sv, kind="stable")
    sv, q = sv[order], q[:, order]
    keep = sv > epsilon
    if not keep.any():
        raise ValueError(f"no eigenvalue of C_0 is above epsilon = {epsilon}")
    L = q[:, keep] / np.sqrt(sv[keep])[None, :]
    cw = L.T @ ct @ L
    lam, r = np.linalg.eigh(0.5 * (cw + cw.T))
    order = np.argsort(-lam, kind="stable")
    lam, r = lam[order], r[:, order]
    u = L @ r
    if kinetic_map:
        u = u * lam[None, :]
    total = float(np.sum(lam * lam))
    cumvar = np.cumsum(lam * lam) / total if total > 0 else np.ones_like(lam)
    d = min(int(np.searchsorted(cumvar, var_cutoff)) + 1, lam.shape[0])
    u = u[:, :d]
    big = np.argmax(np.abs(u), axis=0)
    sign = np.where(u[big, np.arange(d)] < 0, -1.0, 1.0)
    return {"mean": mu, "eigenvalues": lam, "eigenvectors": np.ascontiguousarray(u * sign[None, :]), "cumulative_variance": cumvar, "d": d}


def js_distance_host(p, q) -> float:
    """The Jensen-Shannon distance of two arrays of counts or weights (natural logarithm): ``sqrt((KL(p || m) + KL(q || m)) / 2)`` of the
    normalised ``p`` and ``q``, ``m = (p + q) / 2``, ``0 log 0 = 0``: ``scipy.spatial.distance.jensenshannon(p, q)``, which is what the
    reference reports.  NaN where ``p`` or ``q`` sums to 0."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if p.shape != q.shape:
        raise ValueError(f"p and q differ in shape: {p.shape} and {q.shape}")
    sp, sq = p.sum(), q.sum()
    if not (sp > 0 and sq > 0):
        return float("nan")
    p, q = p / sp, q / sq
    m = (p + q) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        left = np.where(p > 0, p * np.log(p / m), 0.0)
        right = np.where(q > 0, q * np.log(q / m), 0.0)
    return float(np.sqrt((left.sum() + right.sum()) / 2.0))


def tica_js_distances(tic: np.ndarray, ref: np.ndarray, bins_1d: int, bins_2d: int) -> Dict[str, float]:
    """The reference's ``compute_TICA_stats`` for projections ``tic [T, k]`` and ``ref [R, k]`` (finite rows, ``k`` = 1 or 2 components):
    ``js_distance_tic0`` from ``np.histogram`` over the common range of the first component, and with two components
    ``js_distance_tic01`` from ``np.histogram2d`` over the common ranges of both.  NaN where ``tic`` has no row."""
    out = {}
    if tic.shape[0] == 0 or ref.shape[0] == 0:
        out["js_distance_tic0"] = float("nan")
        if tic.shape[1] >= 2:
            out["js_distance_tic01"] = float("nan")
        return out
    r0 = (min(ref[:, 0].min(), tic[:, 0].min()), max(ref[:, 0].max(), tic[:, 0].max()))
    out["js_distance_tic0"] = js_distance_host(np.histogram(ref[:, 0], range=r0, bins=bins_1d)[0], np.histogram(tic[:, 0], range=r0, bins=bins_1d)[0])
    if tic.shape[1] >= 2:
        r1 = (min(ref[:, 1].min(), tic[:, 1].min()), max(ref[:, 1].max(), tic[:, 1].max()))
        hr = np.histogram2d(ref[:, 0], ref[:, 1], range=(r0, r1), bins=bins_2d)[0]
        ht = np.histogram2d(tic[:, 0], tic[:, 1], range=(r0, r1), bins=bins_2d)[0]
        out["js_distance_tic01"] = js_distance_host(hr.flatten(), ht.flatten())
    return out


def tica_feature_table(mol: dict, features: str = "all") -> Tuple[np.ndarray, List[str]]:
    """``(index int32 [F, 4], labels [2 F])`` of the TICA features of ``mol``: phi and psi of every residue (pyemma's backbone torsions: no
    omega) and, with ``features="all"``, chi1..chi4; the labels name the interleaved columns ``COS(...)``, ``SIN(...)``."""
    if features not in ("all", "backbone"):
        raise ValueError(f"features must be 'all' or 'backbone', got {features!r}")
    index, labels = torsion_indices(mol, backbone=True, sidechain=features == "all")
    keep = [i for i, l in enumerate(labels) if not l.startswith("OMEGA ")]
    columns = [f"{fn}({labels[i]})" for i in keep for fn in ("COS", "SIN")]
    return np.ascontiguousarray(index[keep], dtype=np.int32).reshape(-1, 4), columns


# ---- the meter -------------------------------------------------------------------------------------------------------------------------------

class TICAMetrics(TrajectoryMeter):
    """The meter of one dataset (the ``TrajectoryMetric`` protocol `callbacks.TrajectoryMetricCallback` drives): a TICA model fitted on the
    reference trajectory, and per chain and for the joined trajectory the projection on its first two components, the Jensen-Shannon
    distances of their histograms from the reference's, and the autocovariance of the first component, written under
    ``<output_dir>/<label>/tica/`` on rank 0:

        model.json      feature labels and atom indices, lag, d, the options, and ``note``: why no model was fitted, or null
        model.npz       mean [W], eigenvalues [m], eigenvectors [W, d], cumulative_variance [m]
        true_traj.npz   tic01 [R, min(d, 2)], autocov [max_acf_lag + 1], num_frames: the reference projected on its own model
        <i>.npz         per chain: tic01 [T, min(d, 2)], js_distance_tic0, js_distance_tic01 (omitted when d < 2), autocov
                        [max_acf_lag + 1], num_frames, nonfinite_frames
        joined.npz      the same for all chains so far in running order

    The reference comes from ``reference`` (frames ``[T, n, 3]``, or the path of such an ``.npy``) if given, else from the dataset's own
    frames ``dataset.xyz``.  It is featurised in chunks that overlap by ``lag`` frames, so that a chunk boundary loses no lag pair; the
    moments of the chunks are summed, the model is fitted on the host (`fit_tica`).  Without a reference, with one of at most ``lag``
    frames, or with one that has a non-finite feature no model is fitted: ``model.json`` carries the reason in ``note``, nothing else is
    written and `compute` returns ``{}``.

    Rows of a chain with a non-finite feature are counted as ``nonfinite_frames`` and left out of the histograms; such a chain's
    autocovariance is NaN.  ``js_distance_tic0`` is ``np.histogram`` with ``bins_1d`` bins over the range min / max of reference and
    trajectory, ``js_distance_tic01`` ``np.histogram2d`` with ``bins_2d`` bins: exactly the reference's ``compute_TICA_stats``; the
    histograms run on the host (two columns).  ``autocov[k]`` is ``sum_t y_t y_{t+k} / (T - k)`` of the first component (NaN for
    ``k >= T``).  THE JOINED AUTOCOVARIANCE is the sum of the chains' sums over the sum of their counts, never the autocovariance of the
    concatenated frames: no pair crosses from one chain into the next.  A chain with a non-finite frame is left out of it.

    ``device``: ``"auto"`` takes the device path (``native.internal_coords`` with ``cossin``, ``native.lagged_moments``,
    ``native.project_frames``, ``native.autocov_sums``; of a chain only its first two components and ``max_acf_lag + 1`` sums come
    back) for float32 sample tensors on a GPU when the native library loads, the features have at most 128 columns and
    ``max_acf_lag <= 4096``, else the host path.  ``"host"`` forces the host path, ``"device"`` makes a missing device path an error.
    `compute` returns ``{"<label>/tica/js_distance_tic0_joined": the joined trajectory's value}``."""

    DIRECTORY = "tica"
    REFERENCE_CHUNK = 1 << 18  # lag pairs of the reference trajectory taken at a time

    def __init__(self, dataset, lag: int = 1000, max_acf_lag: int = 1000, features: str = "all", bins_1d: int = 100, bins_2d: int = 50,
                 var_cutoff: float = 0.95, epsilon: float = 1e-6, kinetic_map: bool = True, reference=None, device: str = "auto",
                 output_dir: str = "sampler", sample_key: str = "xhat_traj", **_):
        super().__init__(dataset, sample_key, output_dir, device)
        for name, value, low in (("lag", lag, 1), ("max_acf_lag", max_acf_lag, 0), ("bins_1d", bins_1d, 1), ("bins_2d", bins_2d, 1)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low:
                raise ValueError(f"{name} must be an integer of at least {low}, got {value!r}")
        mol = getattr(dataset, "molecule", None)
        if mol is None:
            raise ValueError(f"TICAMetrics: the dataset of label {dataset.label()!r} has no molecule to find torsions in")
        self.lag, self.max_acf_lag, self.bins_1d, self.bins_2d = int(lag), int(max_acf_lag), int(bins_1d), int(bins_2d)
        self.features = features
        self.var_cutoff, self.epsilon, self.kinetic_map = float(var_cutoff), float(epsilon), bool(kinetic_map)
        self.reference = reference
        self.n_atoms = len(mol["atom_names"])
        self.index, self.feature_labels = tica_feature_table(mol, features)
        self.width = len(self.feature_labels)
        self.model: Optional[Dict[str, np.ndarray]] = None
        self.note: Optional[str] = None
        self._ref_tic01: Optional[np.ndarray] = None
        self._chains: List[dict] = []  # per chain on the host: tic01, finite mask, sums, counts
        self._last_joined: Optional[float] = None

    def _device_fits(self) -> bool:
        return 1 <= self.width <= TICA_MAX_WIDTH and self.max_acf_lag <= TICA_MAX_ACF_LAG

    def _device_needs(self) -> str:
        return (f"TICAMetrics(device='device') needs float32 sample tensors on a GPU, 1 to {TICA_MAX_WIDTH} feature columns (these are "
                f"{self.width}) and max_acf_lag <= {TICA_MAX_ACF_LAG}")

    # ---- the two paths: tensors on the device path, arrays on the host path ------------------------------------------------------------------

    def _uploaded(self, dev):
        if dev not in self._dev:  # (index, mean, eigenvectors)
            self._dev[dev] = [torch.from_numpy(self.index).to(dev), None, None]
        if self._dev[dev][1] is None and self.model is not None:
            self._dev[dev][1] = torch.from_numpy(self.model["mean"]).to(dev)
            self._dev[dev][2] = torch.from_numpy(self.model["eigenvectors"]).to(dev)
        return self._dev[dev]

    def _features(self, frames):
        """Raw frames ``[T, n, 3]`` -> the feature rows ``[T, W]`` in float32: a device tensor on the device path, an array on the host path."""
        if int(frames.shape[1]) != self.n_atoms:
            raise ValueError(f"the frames of {self.label!r} must have {self.n_atoms} atoms, got {tuple(frames.shape)}")
        if self._device_path(frames):
            from . import native

            return native.internal_coords(frames, self._uploaded(frames.device)[0], cossin=True)
        return internal_coords_host(frames, self.index, cossin=True).astype(np.float32)

    def _moments(self, x) -> Tuple[np.ndarray, np.ndarray]:
        if torch.is_tensor(x):
            from . import native

            s, m = native.lagged_moments(x, self.lag)
            return s.cpu().numpy(), m.cpu().numpy()
        return lagged_moments_host(x, self.lag)

    def _project(self, x):
        """Feature rows -> (the projection [T, d] where it was computed, the rows with a non-finite feature as a count)."""
        if torch.is_tensor(x):
            from . import native

            _, mean, v = self._uploaded(x.device)
            return native.project_frames(x, mean, v), int((~torch.isfinite(x).all(dim=1)).sum().item())
        return project_host(x, self.model["mean"], self.model["eigenvectors"]), int((~np.isfinite(x).all(axis=1)).sum())

    def _autocov_sums(self, proj):
        """The projection -> the autocovariance sums of its first column, on the host."""
        if torch.is_tensor(proj):
            from . import native

            return native.autocov_sums(proj[:, 0], self.max_acf_lag).cpu().numpy()
        return autocov_sums_host(proj[:, 0], self.max_acf_lag)

    @staticmethod
    def _host(a) -> np.ndarray:
        return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

    # ---- protocol ------------------------------------------------------------------------------------------------------------------------------

    def _fit(self, ref) -> Optional[str]:
        """Fits `model` on the reference frames; returns the reason where it cannot."""
        if self.width == 0:
            return "the molecule has no phi, psi or chi torsion: no feature to fit on"
        if ref is None:
            return "no reference frames (neither dataset.xyz nor reference=): no model is fitted and nothing is measured"
        R = int(ref.shape[0])
        if R <= self.lag:
            return f"the reference has {R} frames, the lag is {self.lag}: no lag pair to fit on"
        n_pairs = R - self.lag
        sums = np.zeros((2, self.width))
        moments = np.zeros((3, self.width, self.width))
        for p0 in range(0, n_pairs, self.REFERENCE_CHUNK):  # pairs p0 <= t < p1 need the frames p0 .. p1 + lag - 1: the chunks overlap by `lag`
            p1 = min(n_pairs, p0 + self.REFERENCE_CHUNK)
            s, m = self._moments(self._features(self._on_compute_device(ref[p0 : p1 + self.lag])))
            sums += s
            moments += m
        if not (np.isfinite(sums).all() and np.isfinite(moments).all()):
            return "the reference has a non-finite feature (a frame with a non-finite coordinate): no model is fitted"
        try:
            self.model = fit_tica(sums, moments, n_pairs, self.epsilon, self.var_cutoff, self.kinetic_map)
        except ValueError as e:
            return f"the fit failed: {e}"
        return None

    def on_sample_start(self):
        ref = self._reference_frames(self.n_atoms, "the reference frames of", self.reference)
        self.note = self._fit(ref)
        true = None
        if self.model is not None:
            R = int(ref.shape[0])
            tic01, col0 = [], []
            for t0 in range(0, R, self.REFERENCE_CHUNK):
                proj, _ = self._project(self._features(self._on_compute_device(ref[t0 : t0 + self.REFERENCE_CHUNK])))
                tic01.append(self._host(proj[:, :2]))
                col0.append(proj[:, 0])
            y = torch.cat(col0) if torch.is_tensor(col0[0]) else np.concatenate(col0)
            sums = self._autocov_sums(y[:, None])
            self._ref_tic01 = np.concatenate(tic01)
            true = {"tic01": self._ref_tic01, "autocov": autocov_from_sums(sums, autocov_counts(R, self.max_acf_lag)),
                    "num_frames": np.asarray(R, dtype=np.int64)}
        if not self._is_rank_zero():
            return
        d = self._dir()
        with open(os.path.join(d, "model.json"), "w") as f:
            json.dump({"feature_labels": self.feature_labels, "atom_indices": self.index.tolist(), "features": self.features, "lag": self.lag,
                       "max_acf_lag": self.max_acf_lag, "bins_1d": self.bins_1d, "bins_2d": self.bins_2d, "var_cutoff": self.var_cutoff,
                       "epsilon": self.epsilon, "kinetic_map": self.kinetic_map, "estimator": "reversible",
                       "d": None if self.model is None else int(self.model["d"]), "note": self.note}, f, indent=1)
        if self.model is not None:
            save_npz(os.path.join(d, "model.npz"), **{k: self.model[k] for k in ("mean", "eigenvalues", "eigenvectors", "cumulative_variance")})
            save_npz(os.path.join(d, "true_traj.npz"), **true)

    def update(self, sample) -> None:
        index, frames, off = self._next_chain(sample)
        T = int(frames.shape[0])
        if T == 0 or self.model is None:
            return
        x = self._features(frames)
        proj, nonfinite = self._project(x)  # (queued on the device path; the count is the one value read here)
        rec = {"index": index, "frames": T, "tic01": proj[:, :2], "nonfinite": nonfinite,
               "sums": self._autocov_sums(proj) if nonfinite == 0 else None}
        self.joined_frames = off + T
        self._pending.append(rec)

    def _arrays(self, tic01: np.ndarray, sums: Optional[np.ndarray], counts: np.ndarray, nonfinite: int) -> dict:
        finite = np.isfinite(tic01).all(axis=1)
        out = {"tic01": tic01}
        out.update({k: np.asarray(v) for k, v in tica_js_distances(tic01[finite], self._ref_tic01, self.bins_1d, self.bins_2d).items()})
        out["autocov"] = np.full(self.max_acf_lag + 1, np.nan) if sums is None else autocov_from_sums(sums, counts)
        out["num_frames"] = np.asarray(tic01.shape[0], dtype=np.int64)
        out["nonfinite_frames"] = np.asarray(nonfinite, dtype=np.int64)
        return out

    def compute(self) -> Dict[str, float]:
        """Brings the first two components of the chains seen since the last call to the host, writes ``<i>.npz`` and ``joined.npz``
        (rank 0) and returns the joined trajectory's Jensen-Shannon distance of the first component."""
        pending, write, d = self._take_pending()
        if self.model is None:
            return {}
        for rec in pending:
            tic01 = np.ascontiguousarray(self._host(rec["tic01"]), dtype=np.float64)
            counts = autocov_counts(rec["frames"], self.max_acf_lag)
            self._chains.append({"tic01": tic01, "sums": rec["sums"], "counts": counts, "nonfinite": rec["nonfinite"]})
            if write:
                save_npz(os.path.join(d, f"{rec['index']}.npz"), **self._arrays(tic01, rec["sums"], counts, rec["nonfinite"]))
        if pending:
            good = [c for c in self._chains if c["sums"] is not None]
            sums = np.sum([c["sums"] for c in good], axis=0) if good else None
            counts = np.sum([c["counts"] for c in good], axis=0) if good else autocov_counts(0, self.max_acf_lag)
            joined = self._arrays(np.concatenate([c["tic01"] for c in self._chains]), sums, counts, sum(c["nonfinite"] for c in self._chains))
            self._last_joined = float(joined["js_distance_tic0"])
            if write:
                save_npz(os.path.join(d, "joined.npz"), **joined)
        return {} if self._last_joined is None else {f"{self.label}/tica/js_distance_tic0_joined": self._last_joined}
